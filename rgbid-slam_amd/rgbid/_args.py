"""The argument checks every binding shares: the one place that says what an integer, a number that reaches the library as a float32, a
device tensor and a device pointer are.  A module's public `*_arg` functions name their argument and its range and call these; they keep
their own message texts, which tests/test_cpu_binding_args.py pins."""
import ctypes as C
import math

import numpy as np
import torch


def integer(name, v):
    """-> v as an int: a Python or numpy integer, no bool (ValueError otherwise)"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name}: an integer, got {v!r}")
    return int(v)


def in_range(name, n, lo, hi, span, got):
    """-> n when lo <= n <= hi; `span` is how the message writes the range, `got` the argument as the caller gave it"""
    if not lo <= n <= hi:
        raise ValueError(f"{name} must lie in {span}, got {got!r}")
    return n


def integer_in(name, v, lo, hi, span):
    """-> v as an int in lo .. hi (ValueError otherwise)"""
    return in_range(name, integer(name, v), lo, hi, span, v)


def float32(v, what, reject=(), over="ignore"):
    """-> v as the float32 value the library receives, as a float; ValueError(what) for what numpy takes for no number and for an instance
    of `reject`.  over: numpy's overflow mode for a value beyond float32's range, which comes back infinite"""
    try:
        if isinstance(v, reject):
            raise TypeError
        with np.errstate(over=over):
            return float(np.float32(v))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(what) from None


def finite32(name, v):
    """-> v as a finite float32 value (ValueError otherwise)"""
    f = float32(v, f"{name}: a number, got {v!r}")
    if not math.isfinite(f):
        raise ValueError(f"{name} must be finite, got {v!r}")
    return f


def finite64(name, v):
    """-> v as a finite float, no bool and no str (ValueError otherwise)"""
    try:
        f = float(v)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{name}: a number, got {v!r}") from None
    if isinstance(v, (bool, str)) or not math.isfinite(f):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return f


def positive32(name, v, what, reject=(), over="ignore"):
    """-> v as a finite float32 value > 0 (ValueError otherwise; `what`, `reject` and `over` are float32's)"""
    f = float32(v, what, reject, over)
    if not (math.isfinite(f) and f > 0):
        raise ValueError(f"{name} must be finite and > 0, got {v!r}")
    return f


def int4(x):
    """the dtype test of an index tensor: 4-byte integers, int32 holding uint32 bits"""
    return x.element_size() == 4 and not x.is_floating_point()


def on_device(name, x, device):
    """-> x when `device` is None or the index of x's device (ValueError otherwise)"""
    if device is not None and x.device.index != device:
        raise ValueError(f"{name} must live on device {device}")
    return x


def cuda_tensor(name, x, dtype, shape, what, device=None):
    """-> x when it is a contiguous CUDA tensor of `dtype` (a torch dtype, or a test such as int4) and of `shape` (None: any extent), on
    `device` when given; ValueError(what) otherwise"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and (dtype(x) if callable(dtype) else x.dtype == dtype) and x.dim() == len(shape)
            and all(s is None or s == n for s, n in zip(shape, x.shape)) and x.is_contiguous()):
        raise ValueError(what)
    return on_device(name, x, device)


def rows3(name, x, dtype, rows=None, device=None):
    """-> x: a contiguous CUDA tensor [n, 3] of `dtype`, of `rows` rows when given (ValueError otherwise)"""
    cuda_tensor(name, x, dtype, (None, 3), f"{name}: a contiguous CUDA {'int32' if dtype is int4 else str(dtype)[6:]} tensor [n, 3]")
    if rows is not None and x.shape[0] != rows:
        raise ValueError(f"{name}: {rows} rows, one per vertex, got {x.shape[0]}")
    return on_device(name, x, device)


def ptr(x):
    """the device pointer of a tensor as the library takes it: NULL for an empty one"""
    return C.c_void_p(x.data_ptr() if x.numel() else 0)


def opt_ptr(x):
    """ptr, and NULL for None"""
    return C.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)
