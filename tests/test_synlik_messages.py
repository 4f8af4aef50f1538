"""CPU: the exception type and the full text of every kind of invalid call of the synthetic-likelihood functions
(elfi_amd/synlik.py) that is refused in Python, before the library is reached: the batched calls, the one-group callables
and their factories, and select_penalty / log_SL_stdev with a model that must not be reached.  Calls with two faults pin
which one is reported.  The texts were recorded from the code as it stood before its call shape was written once; they are
what users and the reference's callers see, so a change of the code keeps them character for character.
"""
import numpy as np
import pytest

import elfi_amd as E
from elfi_amd import _lib, synlik as S

VE, NI = ValueError, NotImplementedError
RIDGE = "unknown shrinkage 'ridge'"
GLASSO = "graphical-lasso shrinkage is not on the device; shrinkage='warton' is"
NEED_WARTON = "penalties need shrinkage='warton'"
NEED_PENALTY = "shrinkage='warton' needs penalty or penalties"
GAMMA01 = 'Gamma must be between 0 and 1'
EMPTY = 'penalties must be a non-empty list'
PREFIXES = 'prefixes must be ascending row counts >= 2 whose last entry is n=4'
W33 = 'whitening must be (3, 3)'
W_NAN = 'whitening has a non-finite entry'
WIDE65 = '65 summaries: the device kernel takes 1 to 64'
ONE_ROW = 'a group needs at least 2 rows (n=1)'
THIRDS = '4 rows do not divide into 3 groups'
SSY4 = 'ssy has 4 entries, ssx has 3 columns'
ROWS = '16385 rows per group: the semiparametric kernel takes 2 to 16384'
NEED_W = 'the whitened semiparametric likelihood needs a whitening matrix'
NEED_W_KEYWORD = 'the whitened semiparametric likelihood needs whitening='
NO_WSEMI = 'the whitened semiparametric likelihood (wsemiBSL) is not on the device'
NEED_GAMMA = 'the robust likelihood needs gamma'
MEDIAN = "adjustment must be 'mean' or 'variance', not 'median'"
STANDARD_ONLY = 'shrinkage goes with the standard likelihood only (the unbiased and robust ones have none)'
EITHER = 'give either penalty or penalties'
ONE_NUMBER = 'penalty is one number; a list goes to penalties'
GL_PENALTY = 'a graphical-lasso penalty must be non-negative and finite'
GL_EMPTY = 'the penalties must be a number or a non-empty list'
GL_ONLY = "this likelihood is the graphical-lasso one; shrinkage='warton' goes to standard_likelihood"
BATCHED = ("the batched evaluation takes the device likelihoods of elfi_amd (standard_likelihood(...), "
           "semiparametric_likelihood(...), whitened_semiparametric_likelihood(...), unbiased_likelihood()); got 'gaussian'")


class StubModel:
    def generate(self, *args, **kwargs):
        raise AssertionError('the model was reached')


X = np.arange(12.0).reshape(4, 3)
y = np.zeros(3)
W = np.eye(3)
W_WITH_NAN = np.full((3, 3), np.nan)
WIDE = np.zeros((4, 65))
LONG = np.zeros((S.MAX_SEMI_ROWS + 1, 1))
MODEL = StubModel()

CASES = {
    'syn_loglik': [
        (lambda: E.syn_loglik(X, y, shrinkage='ridge', penalty=0.1), VE, RIDGE),
        (lambda: E.syn_loglik(X, y, shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: E.syn_loglik(X, y, penalties=[0.2]), VE, NEED_WARTON),
        (lambda: E.syn_loglik(X, y, shrinkage='warton'), VE, NEED_PENALTY),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalty=1.5), VE, GAMMA01),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalties=[0.2, -0.1]), VE, GAMMA01),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalties=[]), VE, EMPTY),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalties=[[0.1, 0.2]]), VE, EMPTY),
        (lambda: E.syn_loglik(X, y, prefixes=[2, 2, 4]), VE, PREFIXES),
        (lambda: E.syn_loglik(X, y, prefixes=[2, 3]), VE, PREFIXES),
        (lambda: E.syn_loglik(X, y, prefixes=[1, 4]), VE, PREFIXES),
        (lambda: E.syn_loglik(X, y, prefixes=[]), VE, PREFIXES),
        (lambda: E.syn_loglik(X, y, whitening=np.eye(2)), VE, W33),
        (lambda: E.syn_loglik(X, y, whitening=np.ones(3)), VE, W33),
        (lambda: E.syn_loglik(WIDE, np.zeros(65)), VE, WIDE65),
        (lambda: E.syn_loglik(np.zeros((4, 0)), np.zeros(0)), VE, '0 summaries: the device kernel takes 1 to 64'),
        (lambda: E.syn_loglik(X, y, n_groups=4), VE, ONE_ROW),
        (lambda: E.syn_loglik(X, y, n_groups=3), VE, THIRDS),
        (lambda: E.syn_loglik(X, y, n_groups=0), VE, '4 rows do not divide into 0 groups'),
        (lambda: E.syn_loglik(X.reshape(2, 2, 3), y, n_groups=3), VE, 'n_groups=3 but ssx has 2 groups'),
        (lambda: E.syn_loglik(X.reshape(1, 2, 2, 3), y), VE, 'ssx must be 2d (rows of summaries) or 3d (groups of rows)'),
        (lambda: E.syn_loglik(X, np.zeros(4)), VE, SSY4),
        (lambda: E.syn_loglik(X, y, variant='robust'), VE, "variant='robust' needs adjustment='mean' or 'variance'"),
        (lambda: E.syn_loglik(X, y, variant='semi'), VE, "unknown variant 'semi' (standard, unbiased, robust)"),
        (lambda: E.syn_loglik(X, y, adjustment='mean'), VE, NEED_GAMMA),
        (lambda: E.syn_loglik(X, y, adjustment='median', gamma=y), VE, MEDIAN),
        (lambda: E.syn_loglik(X, y, variant='unbiased', adjustment='mean', gamma=y), VE,
         "adjustment='mean' does not go with variant='unbiased'"),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalty=0.2, variant='unbiased'), VE, STANDARD_ONLY),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalty=0.2, adjustment='variance', gamma=y), VE, STANDARD_ONLY),
        # two faults: the shape, then the variant and gamma, then the shrinkage and its penalties, then the prefixes
        (lambda: E.syn_loglik(X, np.zeros(4), variant='semi'), VE, SSY4),
        (lambda: E.syn_loglik(X, y, variant='semi', shrinkage='ridge'), VE, "unknown variant 'semi' (standard, unbiased, robust)"),
        (lambda: E.syn_loglik(X, y, adjustment='mean', shrinkage='ridge'), VE, NEED_GAMMA),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalty=0.2, variant='unbiased', prefixes=[2, 3]), VE, STANDARD_ONLY),
        (lambda: E.syn_loglik(X, y, shrinkage='ridge', variant='unbiased', prefixes=[2, 3]), VE, RIDGE),
        (lambda: E.syn_loglik(X, y, shrinkage='glasso', variant='unbiased'), NI, GLASSO),
        (lambda: E.syn_loglik(X, y, shrinkage='ridge', prefixes=[2, 3]), VE, RIDGE),
        (lambda: E.syn_loglik(X, y, shrinkage='warton', penalty=1.5, prefixes=[2, 3]), VE, GAMMA01),
    ],
    'semi_loglik': [
        (lambda: E.semi_loglik(X, y, shrinkage='ridge', penalty=0.1), VE, RIDGE),
        (lambda: E.semi_loglik(X, y, shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: E.semi_loglik(X, y, penalties=[0.2]), VE, NEED_WARTON),
        (lambda: E.semi_loglik(X, y, shrinkage='warton'), VE, NEED_PENALTY),
        (lambda: E.semi_loglik(X, y, shrinkage='warton', penalty=1.5), VE, GAMMA01),
        (lambda: E.semi_loglik(X, y, shrinkage='warton', penalties=[0.2, -0.1]), VE, GAMMA01),
        (lambda: E.semi_loglik(X, y, shrinkage='warton', penalties=[]), VE, EMPTY),
        (lambda: E.semi_loglik(X, y, prefixes=[2, 2, 4]), VE, PREFIXES),
        (lambda: E.semi_loglik(X, y, prefixes=[2, 3]), VE, PREFIXES),
        (lambda: E.semi_loglik(X, y, prefixes=[1, 4]), VE, PREFIXES),
        (lambda: E.semi_loglik(X, y, prefixes=[]), VE, PREFIXES),
        (lambda: E.semi_loglik(LONG, [0.0]), VE, ROWS),
        (lambda: E.semi_loglik(WIDE, np.zeros(65)), VE, WIDE65),
        (lambda: E.semi_loglik(X, y, n_groups=4), VE, ONE_ROW),
        (lambda: E.semi_loglik(X, y, n_groups=3), VE, THIRDS),
        (lambda: E.semi_loglik(X, np.zeros(4)), VE, SSY4),
        # two faults: the shape, then the row cap, then the shrinkage, then the prefixes
        (lambda: E.semi_loglik(LONG, [0.0], shrinkage='ridge'), VE, ROWS),
        (lambda: E.semi_loglik(LONG, [0.0, 0.0]), VE, 'ssy has 2 entries, ssx has 1 columns'),
        (lambda: E.semi_loglik(X, y, shrinkage='ridge', prefixes=[2, 3]), VE, RIDGE),
    ],
    'wsemi_loglik': [
        (lambda: E.wsemi_loglik(X, y, None), VE, NEED_W),
        (lambda: E.wsemi_loglik(X, y, np.eye(4)), VE, W33),
        (lambda: E.wsemi_loglik(X, y, np.ones(3)), VE, W33),
        (lambda: E.wsemi_loglik(X, y, W_WITH_NAN), VE, W_NAN),
        (lambda: E.wsemi_loglik(X, y, W, shrinkage='ridge', penalty=0.1), VE, RIDGE),
        (lambda: E.wsemi_loglik(X, y, W, shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: E.wsemi_loglik(X, y, W, penalties=[0.2]), VE, NEED_WARTON),
        (lambda: E.wsemi_loglik(X, y, W, shrinkage='warton'), VE, NEED_PENALTY),
        (lambda: E.wsemi_loglik(X, y, W, shrinkage='warton', penalty=1.5), VE, GAMMA01),
        (lambda: E.wsemi_loglik(X, y, W, shrinkage='warton', penalties=[0.2, -0.1]), VE, GAMMA01),
        (lambda: E.wsemi_loglik(X, y, W, prefixes=[2, 2, 4]), VE, PREFIXES),
        (lambda: E.wsemi_loglik(X, y, W, prefixes=[2, 3]), VE, PREFIXES),
        (lambda: E.wsemi_loglik(X, y, W, prefixes=[1, 4]), VE, PREFIXES),
        (lambda: E.wsemi_loglik(LONG, [0.0], np.eye(1)), VE, ROWS),
        (lambda: E.wsemi_loglik(WIDE, np.zeros(65), np.eye(65)), VE, WIDE65),
        (lambda: E.wsemi_loglik(X, y, W, n_groups=4), VE, ONE_ROW),
        (lambda: E.wsemi_loglik(X, y, W, n_groups=3), VE, THIRDS),
        (lambda: E.wsemi_loglik(X, np.zeros(4), W), VE, SSY4),
        # two faults: the shape, then the row cap, then the whitening matrix, then the shrinkage, then the prefixes
        (lambda: E.wsemi_loglik(LONG, [0.0], None), VE, ROWS),
        (lambda: E.wsemi_loglik(X, y, None, shrinkage='ridge'), VE, NEED_W),
        (lambda: E.wsemi_loglik(X, y, np.eye(4), shrinkage='ridge'), VE, W33),
        (lambda: E.wsemi_loglik(X, y, W_WITH_NAN, shrinkage='ridge'), VE, W_NAN),
        (lambda: E.wsemi_loglik(X, y, W, shrinkage='ridge', prefixes=[2, 3]), VE, RIDGE),
    ],
    'glasso_loglik': [
        (lambda: E.glasso_loglik(X, y), VE, EITHER),
        (lambda: E.glasso_loglik(X, y, penalty=0.1, penalties=[0.1]), VE, EITHER),
        (lambda: E.glasso_loglik(X, y, penalty=[0.1, 0.2]), VE, ONE_NUMBER),
        (lambda: E.glasso_loglik(X, y, penalty=-0.1), VE, GL_PENALTY),
        (lambda: E.glasso_loglik(X, y, penalties=[]), VE, GL_EMPTY),
        (lambda: E.glasso_loglik(X, y, penalties=[0.1, np.inf]), VE, GL_PENALTY),
        (lambda: E.glasso_loglik(X, y, penalty=0.1, tol=0.0), VE, 'tol must be positive'),
        (lambda: E.glasso_loglik(X, y, penalty=0.1, max_iter=0), VE, 'max_iter=0: 1 to 1048576'),
        (lambda: E.glasso_loglik(X, y, penalty=0.1, whitening=np.eye(2)), VE, W33),
        (lambda: E.glasso_loglik(WIDE, np.zeros(65), penalty=0.1), VE, WIDE65),
        (lambda: E.glasso_loglik(X, y, penalty=0.1, n_groups=4), VE, ONE_ROW),
        (lambda: E.glasso_loglik(X, y, penalty=0.1, n_groups=3), VE, THIRDS),
        (lambda: E.glasso_loglik(X, np.zeros(4), penalty=0.1), VE, SSY4),
        # two faults: the shape, then the penalties, then the whitening matrix
        (lambda: E.glasso_loglik(X, np.zeros(4), penalty=-0.1), VE, SSY4),
        (lambda: E.glasso_loglik(X, y, penalty=-0.1, whitening=np.eye(2)), VE, GL_PENALTY),
    ],
    'one_group': [
        (lambda: S.gaussian_syn_likelihood(X, y, shrinkage='ridge'), VE, RIDGE),
        (lambda: S.gaussian_syn_likelihood(X, y, shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: S.gaussian_syn_likelihood(X, y, shrinkage='warton'), VE, NEED_PENALTY),
        (lambda: S.gaussian_syn_likelihood(X, y, shrinkage='warton', penalty=1.5), VE, GAMMA01),
        (lambda: S.gaussian_syn_likelihood(X, y, penalty=0.5, whitening=np.eye(2)), VE, W33),
        (lambda: S.gaussian_syn_likelihood(X, np.zeros(4)), VE, SSY4),
        (lambda: S.gaussian_syn_likelihood(X[:1], y), VE, ONE_ROW),
        (lambda: S.gaussian_syn_likelihood_ghurye_olkin(X, np.zeros(4)), VE, SSY4),
        (lambda: S.gaussian_syn_likelihood_ghurye_olkin(WIDE, np.zeros(65)), VE, WIDE65),
        (lambda: S.syn_likelihood_misspec(X, y, None, 'mean'), VE, NEED_GAMMA),
        (lambda: S.syn_likelihood_misspec(X, y, y, 'median'), VE, MEDIAN),
        (lambda: S.syn_likelihood_misspec(X, np.zeros(4), y, 'variance'), VE, SSY4),
        (lambda: S.semi_param_kernel_estimate(X, y, whitening=W), NI, NO_WSEMI),
        (lambda: S.semi_param_kernel_estimate(X, y, shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: S.semi_param_kernel_estimate(X, y, shrinkage='ridge'), VE, RIDGE),
        (lambda: S.semi_param_kernel_estimate(X, y, shrinkage='warton'), VE, NEED_PENALTY),
        (lambda: S.semi_param_kernel_estimate(LONG, [0.0]), VE, ROWS),
        (lambda: E.wsemi_param_kernel_estimate(X, y), VE, NEED_W_KEYWORD),
        (lambda: E.wsemi_param_kernel_estimate(X, y, whitening=np.eye(2)), VE, W33),
        (lambda: E.wsemi_param_kernel_estimate(X, y, whitening=W_WITH_NAN), VE, W_NAN),
        (lambda: E.wsemi_param_kernel_estimate(X, y, shrinkage='glasso', penalty=0.1, whitening=W), NI, GLASSO),
        (lambda: E.wsemi_param_kernel_estimate(X, y, shrinkage='warton', penalty=1.5, whitening=W), VE, GAMMA01),
        (lambda: S.gaussian_syn_likelihood_glasso(X, y, shrinkage='warton', penalty=0.1), VE, GL_ONLY),
        (lambda: S.gaussian_syn_likelihood_glasso(X, y), VE, EITHER),
        (lambda: S.gaussian_syn_likelihood_glasso(X, y, penalty=[0.1, 0.2]), VE, ONE_NUMBER),
        (lambda: S.gaussian_syn_likelihood_glasso(X, y, penalty=0.1, whitening=np.eye(2)), VE, W33),
        (lambda: S.gaussian_syn_likelihood_glasso(X, np.zeros(4), penalty=0.1), VE, SSY4),
    ],
    'factories': [
        (lambda: E.standard_likelihood(shrinkage='ridge'), VE, RIDGE),
        (lambda: E.standard_likelihood(shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: E.standard_likelihood()(X, y, shrinkage='glasso'), NI, GLASSO),
        (lambda: E.standard_likelihood(shrinkage='warton')(X, y), VE, NEED_PENALTY),
        (lambda: E.semiparametric_likelihood(shrinkage='ridge'), VE, RIDGE),
        (lambda: E.semiparametric_likelihood(shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: E.semiparametric_likelihood(whitening=W), NI, NO_WSEMI),
        (lambda: E.semiparametric_likelihood(shrinkage='ridge', whitening=W), VE, RIDGE),
        (lambda: E.semiparametric_likelihood()(X, y, whitening=W), NI, NO_WSEMI),
        (lambda: E.whitened_semiparametric_likelihood(None), VE, NEED_W),
        (lambda: E.whitened_semiparametric_likelihood(W, shrinkage='ridge'), VE, RIDGE),
        (lambda: E.whitened_semiparametric_likelihood(W, shrinkage='glasso', penalty=0.1), NI, GLASSO),
        (lambda: E.whitened_semiparametric_likelihood(None, shrinkage='ridge'), VE, RIDGE),
        (lambda: E.whitened_semiparametric_likelihood(W)(X, y, whitening=None), VE, NEED_W_KEYWORD),
        (lambda: E.whitened_semiparametric_likelihood(np.eye(2))(X, y), VE, W33),
        (lambda: E.unbiased_likelihood()(X, np.zeros(4)), VE, SSY4),
        (lambda: E.robust_likelihood('median'), VE, MEDIAN),
        (lambda: E.robust_likelihood('mean')(X, y, None), VE, NEED_GAMMA),
        (lambda: E.glasso_likelihood(-1.0), VE, GL_PENALTY),
        (lambda: E.glasso_likelihood([]), VE, GL_EMPTY),
        (lambda: E.glasso_likelihood(0.1)(X, y, shrinkage='warton'), VE, GL_ONLY),
    ],
    'tools': [
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], shrinkage='glasso'), NI, GLASSO),
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], shrinkage=None), VE, 'unknown shrinkage None'),
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], shrinkage='ridge'), VE, RIDGE),
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], likelihood='gaussian'), TypeError, BATCHED),
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], likelihood='gaussian', shrinkage='ridge'), VE, RIDGE),
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], likelihood=E.semiparametric_likelihood(), whitening=W), NI, NO_WSEMI),
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], likelihood=E.semiparametric_likelihood(), shrinkage='glasso'), NI,
         GLASSO),
        (lambda: E.select_penalty(MODEL, 4, [0.5], ['S1'], likelihood=S.wsemi_param_kernel_estimate), VE, NEED_W_KEYWORD),
        (lambda: E.log_SL_stdev(MODEL, [0.5], [4], ['S1'], likelihood='gaussian'), TypeError, BATCHED),
        (lambda: E.log_SL_stdev(MODEL, [0.5], [4], ['S1'], likelihood=S.wsemi_param_kernel_estimate), VE, NEED_W_KEYWORD),
    ],
}

FLAT = [(call, exc, text) for group in CASES.values() for call, exc, text in group]
IDS = ['%s-%d' % (name, i) for name, group in CASES.items() for i in range(len(group))]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', refuse)


@pytest.mark.parametrize('call, exc, text', FLAT, ids=IDS)
def test_invalid_call_is_refused_with_its_recorded_type_and_text(call, exc, text):
    with pytest.raises(exc) as raised:
        call()
    assert type(raised.value) is exc and str(raised.value) == text
