"""What the row calls (sushi_amd/retime.py, envelope.py, filter.py: a 1-D row of samples in, a 1-D row out) check alike, stated
once.  Host only: torch is imported where a tensor is looked at.  `who` is the caller's prefix of every SushiError text."""
import numpy as np

from . import _native
from .common import SushiError

DTYPE_CODE = {np.dtype(np.uint8): _native.U8, np.dtype(np.float32): _native.F32}     # a sample type's SUSHI_HIP_U8 / _F32
MAX_OUT_LEN = 1 << 40        # out_len of a call stays below it


def host_row(who, samples):
    """samples as a 1-D uint8 / float32 array."""
    x = np.asarray(samples)
    if x.ndim != 1 or x.dtype not in DTYPE_CODE:
        raise SushiError("%s: a 1-D uint8 or float32 array" % who)
    return x


def device_row(who, tensor):
    """The dtype code of a contiguous 1-D uint8 / float32 CUDA tensor."""
    import torch
    codes = {torch.uint8: _native.U8, torch.float32: _native.F32}
    if not isinstance(tensor, torch.Tensor) or tensor.dim() != 1 or not tensor.is_cuda or not tensor.is_contiguous() or \
            tensor.dtype not in codes:
        raise SushiError("%s: a contiguous 1-D uint8 or float32 CUDA tensor" % who)
    return codes[tensor.dtype]


def device_out(who, tensor, out, out_len=None):
    """out must be a contiguous 1-D CUDA tensor (or view) of tensor's dtype and device; of out_len samples where that is given."""
    import torch
    if not isinstance(out, torch.Tensor) or out.dim() != 1 or out.dtype != tensor.dtype or out.device != tensor.device or \
            not out.is_contiguous() or (out_len is not None and int(out.shape[0]) != out_len):
        raise SushiError("%s: out must be a contiguous 1-D CUDA tensor of the input's dtype and device%s"
                         % (who, "" if out_len is None else " with out_len samples"))


def row_span(who, n_in, in_start, out_len):
    """in_start lies in the input of n_in samples, and there are 1 .. 2^40 - 1 outputs."""
    if n_in < 1 or not 0 <= in_start <= n_in - 1:
        raise SushiError("%s: in_start lies outside the input" % who)
    if not 1 <= out_len < MAX_OUT_LEN:
        raise SushiError("%s: 1 .. 2^40 - 1 outputs" % who)
