"""NumPy reference of lh_integrate_dense's interpolant (include/landhydro.h): the cubic
Hermite polynomial through (y0, f0) at theta = 0 and (y1, f1) at theta = 1 of a step of size h."""
import numpy as np


def hermite(theta, h, y0, y1, f0, f1):
    """u(theta) = (1 - theta) y0 + theta y1 + theta (theta - 1) ((1 - 2 theta)(y1 - y0) + (theta - 1) h f0 + theta h f1)
    in Float64, written as the library evaluates it: exactly y0 at theta = 0 and y1 at theta = 1."""
    theta = np.float64(theta)
    h = np.float64(h)
    y0, y1, f0, f1 = (np.asarray(a, dtype=np.float64) for a in (y0, y1, f0, f1))
    inner = (1.0 - 2.0 * theta) * (y1 - y0) + ((theta - 1.0) * h) * f0 + (theta * h) * f1
    return (1.0 - theta) * y0 + theta * y1 + (theta * (theta - 1.0)) * inner
