"""Launch helpers every wrapper over the C ABI shares: tensor checks, device pointers, the current stream, byte workspaces."""
import ctypes
from typing import Optional, Sequence

import torch

from . import lib as _l


def _dev(t: torch.Tensor, name: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be a torch.Tensor')
    if not t.is_cuda:
        raise _l.SunerfHipError(f'{name} is on {t.device}: the fused renderer has no CPU path '
                                '(move the module and its inputs to a ROCm device)')
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be float32, got {t.dtype}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {tuple(shape)}')
    return t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(cache, dev, nbytes: int) -> torch.Tensor:
    """The byte workspace ``cache`` keeps for the current stream of ``dev``, grown to at least ``nbytes``."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def _ptr_array(tensors: Sequence[torch.Tensor]):
    """The host array of device pointers the C ABI takes for per-layer tensor lists."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
