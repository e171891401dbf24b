"""The one way this package calls a stream-taking entry point of liblapwarm_hip (lap/_hip.py)."""
from __future__ import annotations

import torch
from torch._C import _cuda_getCurrentRawStream  # the handle itself: no torch.cuda.Stream object per call

from lap import _hip


def hip_call(symbol: str, what: str, device, *args) -> None:
    """lib.<symbol>(*args, stream) with the current torch stream of `device` (a tensor's device: it has its
    index) as the last argument.  A tensor passes its address and None a null pointer; anything else goes to
    ctypes as it is.  `what` names the caller in the exceptions of _hip.check (HIP runtime errors, n above the
    limit); any other nonzero code raises RuntimeError with the library's error text.  Only enqueues: no
    synchronisation, no allocation."""
    rc = getattr(_hip.load(), symbol)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                                      _cuda_getCurrentRawStream(device.index))
    if _hip.check(rc, what) != 0:
        raise RuntimeError(f"{symbol} failed (code {rc}): {_hip.last_error()}")
