"""The integer IQ output of the two synthesisers (include/lorahip.h, "Integer IQ output") restated in numpy, for the tests: per component
t = float32(scale) * c in fp32, r = rint(t) (ties to even), stored 0 for NaN, lo for r < lo, hi for r > hi, int(r) otherwise; a component
is clipped when r is NaN or outside [lo, hi]."""
import numpy as np

BOUNDS = {"sc16": (-32768, 32767), "sc8": (-128, 127)}
DTYPES = {"sc16": np.int16, "sc8": np.int8}
DEFAULT_SCALE = {"sc16": 32767.0, "sc8": 127.0}


def quantise(values, fmt, scale):
    """(integers of the format's dtype, number of clipped components) of float32 `values` (any shape; complex64 is read as I, Q pairs)"""
    lo, hi = BOUNDS[fmt]
    c = np.ascontiguousarray(values)
    if np.iscomplexobj(c):
        c = c.astype(np.complex64).view(np.float32).reshape(c.shape + (2,))
    c = c.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (np.float32(scale) * c).astype(np.float32)             # one fp32 multiply
        r = np.rint(t)
    nan = np.isnan(r)
    clipped = nan | (r < lo) | (r > hi)
    q = np.where(nan, np.float32(0), np.clip(r, lo, hi))           # clip maps -Inf / +Inf to lo / hi
    return q.astype(DTYPES[fmt]), int(clipped.sum())
