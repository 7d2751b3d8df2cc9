"""Helpers the bindings share for handing tensors and arrays to the C ABI.
torch is imported only where a tensor is made or its stream looked up."""
from __future__ import annotations

import numpy as np


def _ptr(x):
    """Device pointer of a torch tensor / int / None."""
    if x is None or isinstance(x, int):
        return x
    return x.data_ptr()


def _hptr(x):
    """Host pointer of a numpy array / CPU torch tensor / int / None."""
    if x is None or isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data


def _stream(stream, *tensors):
    if stream is not None:
        return stream if isinstance(stream, int) else stream.cuda_stream
    for t in tensors:
        if t is not None and not isinstance(t, int) and getattr(t, "is_cuda", False):
            import torch
            return torch.cuda.current_stream(t.device).cuda_stream
    return None


def _pack(packets):
    lens = np.array([len(p) for p in packets], np.uint32)
    off = np.zeros(len(packets), np.uint64)
    if len(packets) > 1:
        np.cumsum(lens[:-1], out=off[1:])
    buf = np.frombuffer(b"".join(bytes(p) for p in packets) + bytes(16), np.uint8).copy()
    return buf, off, lens


def _to(dev, a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(dev)   # writable copy (torch warns on read-only arrays)


def _records(t, dtype):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype)
