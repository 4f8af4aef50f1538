"""The AR(1) example (elfi/examples/ar1.py) stated in NumPy: what csrc/series.hip's ar1_kernel computes (include/elfihip.h:
elfihip_ar1_series) -- x_0 = 0, x_i = phi x_{i-1} + w_i, the product rounded before the sum -- and the distance on the series."""
import numpy as np


def noise_from_state(random_state, batch, n_obs):
    """The reference's one draw: randn(batch, n_obs + 1); column 0 is drawn and unused."""
    return random_state.randn(batch, n_obs + 1)


def series(phi, W):
    """X (n, n_obs) for the noise W (n, n_obs + 1)."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    n, L = W.shape
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64).reshape(-1), (n,))
    x = np.zeros((n, L))
    prev = np.zeros(n)
    with np.errstate(all='ignore'):
        for i in range(1, L):
            x[:, i] = phi * prev + W[:, i]
            prev = x[:, i]
    return x[:, 1:]
