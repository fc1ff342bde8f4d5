"""What the ctypes mirrors of the half-length real-row libraries share beside the loader of _addon.py (dct, hilbert, mdct, stft, welch, bands): the
check of a tensor argument and the host round trip of the array forms.  Private: the mirrors' public names stay their own."""
import numpy as np


def check_tensor(x, what, dtype=None, axes=1):
    """x if it is a contiguous torch tensor of dtype (None: float32) with at least `axes` axes; TypeError / ValueError otherwise"""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what} must be a torch tensor on the device, not {type(x).__name__}")
    if x.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, not {x.dtype}")
    if x.ndim < axes or not x.is_contiguous():
        raise ValueError(f"{what} must be contiguous with at least " + ("one axis" if axes == 1 else f"{axes} axes"))
    return x


def host_round_trip(x, out_dtype, launch, what):
    """x: (batch, n) contiguous float32 on the host -> (batch, n) of out_dtype from launch(d_in, d_out) (the library's status) on the
    null stream: upload, one launch, synchronize, download.  A status that is not 0 raises RuntimeError(`what` -> status)"""
    from . import api      # the device allocator and the copies of libsmfft_amd.so
    size = np.dtype(out_dtype).itemsize
    din, dout = api.DeviceBuffer.from_host(x), api.DeviceBuffer(max(x.size * size, size))
    api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
    rc = launch(din.ptr, dout.ptr)
    if rc == 0:
        rc = api.lib.smfft_synchronize()
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")
    out = dout.to_host(out_dtype, x.shape)
    for buf in (din, dout):
        buf.free()
    return out
