"""reference src/duwu/sampling/get_sigmas.py: sigma grids for rectified-flow style sampling.  A grid is ``time / (1 - time)`` of a
descending time grid in [min_time, max_time], time = sigma / (1 + sigma); the ``*_time`` functions are the discretisations a
config picks with ``time_disc_func`` (float64 numpy on the host, like the reference)."""
import numpy as np

from uwudiff_amd.sampling import get_sigmas_for_rf as _rf_grid


def uniform_time(min_time, max_time, num_steps):
    """get_sigmas.py:17-18: equally spaced times."""
    return np.linspace(min_time, max_time, num_steps + 1)


def sigmoid_time(min_time, max_time, num_steps, rho=10):
    """get_sigmas.py:21-31: equally spaced in logit(time) (so the result does not depend on rho, as the reference notes), with
    min_time raised to 1e-5 and restored exactly in the first entry."""
    lo = max(min_time, 1e-5)
    logit_lo, logit_hi = np.log(lo / (1 - lo)), np.log(max_time / (1 - max_time))
    r = np.linspace(logit_lo / rho + 0.5, logit_hi / rho + 0.5, num_steps + 1)
    time = 1 / (1 + np.exp(-rho * (r - 0.5)))
    time[0] = lo
    return time


def sigmoid_time_scale(min_time, max_time, num_steps, rho=10):
    """get_sigmas.py:34-41: a sigmoid of slope rho over [-0.5, 0.5], stretched to [0, 1] and then to [min_time, max_time]."""
    time = 1 / (1 + np.exp(-rho * np.linspace(-0.5, 0.5, num_steps + 1)))
    time = (time - time[0]) / (time[-1] - time[0])
    return time * (max_time - min_time) + min_time


def get_sigmas_for_rf(num_steps, max_sigma, min_sigma=0, time_disc_func=None):
    """get_sigmas.py:6-14 (``time_disc_func`` defaults to :func:`uniform_time`)."""
    return _rf_grid(num_steps, max_sigma, min_sigma, time_disc_func or uniform_time)
