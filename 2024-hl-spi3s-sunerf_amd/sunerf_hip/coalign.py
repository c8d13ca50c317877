"""Co-alignment of a view with a prediction of it (include/sunerf_hip_coalign.h, csrc/coalign.hip): the masked
zero-mean normalised cross-correlation over a window of integer shifts, its peak to a fraction of a pixel, and the plate-scale
dict moved by that shift.  The image is never resampled: only ``crpix`` moves.

    found = coalign(observed, predicted, max_shift=8)          # predicted may be NaN where it knows nothing (off the disk)
    grid = shifted_grid(grid, *found['shift'].tolist())

The reduction -- six sums per shift over the pixels valid in both images -- is :func:`shift_sums`, a HIP kernel without a CPU
path.  What follows it (:func:`scores_from_sums`, :func:`peak`) is a few fp64 torch operations on ``(2 my + 1) (2 mx + 1)``
numbers and runs wherever its input lives; nothing waits for the device.  ``ObservationSet.coalign_view`` /
``coalign_views`` apply it to the views of a set."""
from typing import Tuple, Union

import torch

from . import lib as _l
from ._ffi import _ptr, _stream, _workspace

MAX_SHIFT = 32                  # include/sunerf_hip_coalign.h: SUNERF_COALIGN_MAX_SHIFT
N_SUMS = 6                      # n, Sa, Sb, Saa, Sbb, Sab
NO_PEAK, EDGE, FLAT = 1, 2, 4   # status bits of peak()
MEASURES = ('zncc', 'ssd')
BOUNDS = {'zncc': 1.0, 'ssd': 0.0}          # the largest score a measure can give: an exact copy on the pair set
_WORKSPACES = {}


def _window(max_shift) -> Tuple[int, int]:
    pair = tuple(max_shift) if isinstance(max_shift, (tuple, list)) else (max_shift, max_shift)
    if len(pair) != 2 or not all(isinstance(m, int) and not isinstance(m, bool) and 0 <= m <= MAX_SHIFT for m in pair):
        raise ValueError(f'max_shift must be an integer in 0 .. {MAX_SHIFT} or a pair (my, mx) of them, got {max_shift!r}')
    return int(pair[0]), int(pair[1])


def launch(image, template, bad_image, bad_template, my: int, mx: int) -> torch.Tensor:
    """``sunerf_coalign_shift_sums`` on device tensors: ``image`` and ``template`` [C, H, W] float32, the masks uint8 of that
    shape or None.  Returns ``sums`` [C, 2 my + 1, 2 mx + 1, 6] float64."""
    c, h, w = image.shape
    dev = image.device
    sums = torch.empty((c, 2 * my + 1, 2 * mx + 1, N_SUMS), dtype=torch.float64, device=dev)
    if image.numel() == 0:          # the empty call writes nothing
        return sums.zero_()
    with torch.cuda.device(dev):
        nbytes = int(_l.load().sunerf_coalign_workspace_bytes(c, h, w, my, mx))
    ws = _workspace(_WORKSPACES, dev, max(nbytes, 8))
    _l.call(dev, 'sunerf_coalign_shift_sums', _ptr(image), _ptr(template), _ptr(bad_image), _ptr(bad_template), c, h, w, my, mx,
            _ptr(sums), _ptr(ws), _stream(dev))
    return sums


def shift_sums(image: torch.Tensor, template: torch.Tensor, max_shift: Union[int, Tuple[int, int]], bad_image=None,
               bad_template=None) -> torch.Tensor:
    """The six sums of every shift ``(dy, dx)``, ``|dy| <= my``, ``|dx| <= mx``: ``sums[c, dy + my, dx + mx] = n, Sa, Sb, Saa, Sbb,
    Sab`` over the pairs ``a = image[c, r + dy, c + dx]``, ``b = template[c, r, c]`` that lie inside the frame, are both finite and
    are flagged in neither ``bad_image`` nor ``bad_template`` (shape of the image, bool or uint8; not 0 is bad).

    ``image`` and ``template``: [C, H, W] or [H, W] float32 on a ROCm device.  ``max_shift``: an int or ``(my, mx)``, at most 32
    each.  Returns [C, 2 my + 1, 2 mx + 1, 6] float64 on the device, every element written; reruns are bit-identical."""
    my, mx = _window(max_shift)
    for name, t in (('image', image), ('template', template)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'shift_sums: {name} must be a torch.Tensor')
    planes = image[None] if image.dim() == 2 else image
    tpl = template[None] if template.dim() == 2 else template
    if planes.dim() != 3 or planes.dtype != torch.float32:
        raise ValueError(f'shift_sums: image must be float32 [C, H, W] or [H, W], got {image.dtype} {tuple(image.shape)}')
    if tpl.dtype != torch.float32 or tuple(tpl.shape) != tuple(planes.shape):
        raise ValueError(f'shift_sums: template must be float32 of the image\'s shape {tuple(planes.shape)}, got {template.dtype} '
                         f'{tuple(template.shape)}')
    masks = []
    for name, m in (('bad_image', bad_image), ('bad_template', bad_template)):
        if m is not None:
            m = torch.as_tensor(m)
            m = m[None] if m.dim() == 2 else m
            if tuple(m.shape) != tuple(planes.shape):
                raise ValueError(f'{name} must have the shape of the image {tuple(planes.shape)}, got {tuple(m.shape)}')
        masks.append(m)
    if not planes.is_cuda:
        raise _l.SunerfHipError('shift_sums runs on a ROCm device (there is no CPU path)')
    dev = planes.device
    if tpl.device != dev:
        raise ValueError(f'shift_sums: image is on {dev}, template on {tpl.device}')
    masks = [None if m is None else (m.to(dev) != 0).to(torch.uint8).contiguous() for m in masks]
    return launch(planes.contiguous(), tpl.contiguous(), masks[0], masks[1], my, mx)


def scores_from_sums(sums: torch.Tensor, measure: str = 'zncc', min_overlap: float = 0.5) -> torch.Tensor:
    """``sums`` [C, Sy, Sx, 6] -> scores [C, Sy, Sx] float64, larger is better.

    ``'zncc'``: ``cov / sqrt(va * vb)`` with ``cov = n Sab - Sa Sb``, ``va = n Saa - Sa^2``, ``vb = n Sbb - Sb^2``; NaN where
    ``va <= 0`` or ``vb <= 0``.  ``'ssd'``: ``-(Saa - 2 Sab + Sbb) / n``.  Both are NaN where ``n < min_overlap * (the plane's
    largest n over all shifts)`` -- a shift that keeps too little of the frame proves nothing -- and where ``n`` is 0."""
    if measure not in MEASURES:
        raise ValueError(f"measure must be 'zncc' or 'ssd', got {measure!r}")
    if not 0.0 <= float(min_overlap) <= 1.0:
        raise ValueError(f'min_overlap must lie in [0, 1], got {min_overlap!r}')
    if sums.dim() != 4 or sums.shape[-1] != N_SUMS:
        raise ValueError(f'sums must be [C, Sy, Sx, 6], got {tuple(sums.shape)}')
    s = sums.double()
    n, sa, sb, saa, sbb, sab = s.unbind(-1)
    refused = (n < float(min_overlap) * n.amax(dim=(1, 2), keepdim=True)) | (n <= 0)
    if measure == 'zncc':
        cov = n * sab - sa * sb
        va = n * saa - sa * sa
        vb = n * sbb - sb * sb
        refused = refused | (va <= 0) | (vb <= 0)
        score = cov / torch.sqrt(va * vb)
    else:
        score = -((saa - 2.0 * sab) + sbb) / n
    return torch.where(refused, torch.full_like(score, float('nan')), score)


def peak(scores: torch.Tensor, combine: str = 'shared', bound=None) -> dict:
    """The best shift of ``scores`` [C, Sy, Sx] (``Sy = 2 my + 1``, ``Sx = 2 mx + 1``) to a fraction of a pixel.

    ``combine='shared'``: one shift for all planes, from the mean of the planes that have any finite score (an absent channel is
    all NaN and is left out); that map is NaN at a shift where one of the remaining planes is.  ``'planes'``: one per plane.
    The integer peak is the first maximum of the finite scores in row-major order.  Per axis the offset of the parabola through
    the peak and its two neighbours is added: ``0.5 (s- - s+) / (s- - 2 s0 + s+)``, clamped to [-0.5, 0.5].

    Returns ``shift`` ([2] or [C, 2] float64, ``(dy, dx)``), ``integer`` (int64, same shape), ``score`` and ``status`` (int64):
    ``NO_PEAK`` 1: no finite score, shift 0 and score NaN; ``EDGE`` 2: the peak lies on the border of the window in an axis whose
    maximum is above 0, the offset is 0 in that axis -- widen ``max_shift``; ``FLAT`` 4: a neighbour is NaN or the second
    difference is not negative, the offset is 0 in that axis.  An axis whose maximum is 0 has no neighbours: its offset is 0 and
    it sets no bit.

    ``bound``: the largest value the measure can take (``BOUNDS``; None: unknown).  A peak whose score EQUALS it is an exact copy
    on its pair set -- the whole-pixel shift is the answer, and the parabola through it would claim a maximum above the bound
    at a fractional one -- so both offsets are 0 and no bit is set."""
    if combine not in ('shared', 'planes'):
        raise ValueError(f"combine must be 'shared' or 'planes', got {combine!r}")
    if scores.dim() != 3 or scores.shape[1] % 2 != 1 or scores.shape[2] % 2 != 1:
        raise ValueError(f'scores must be [C, 2 my + 1, 2 mx + 1], got {tuple(scores.shape)}')
    m = scores.double()
    sy, sx = m.shape[1], m.shape[2]
    nan = float('nan')
    if combine == 'shared':
        used = torch.isfinite(m).flatten(1).any(dim=1)
        count = used.sum()
        total = torch.where(used[:, None, None], m, torch.zeros_like(m)).sum(dim=0)          # NaN where a used plane is NaN
        m = torch.where(count > 0, total / count, torch.full_like(total, nan))[None]
    p = m.shape[0]
    finite = torch.isfinite(m)
    flat_index = torch.where(finite, m, torch.full_like(m, float('-inf'))).flatten(1).argmax(dim=1)
    found = finite.flatten(1).any(dim=1)
    iy, ix = flat_index // sx, flat_index % sx
    padded = torch.nn.functional.pad(m, (1, 1, 1, 1), value=nan)
    rows = torch.arange(p, device=m.device)
    s0 = padded[rows, iy + 1, ix + 1]
    status = torch.where(found, 0, NO_PEAK).to(torch.int64)
    refine = found if bound is None else found & (s0 != float(bound))
    offsets = []
    for i, size, lo, hi in ((iy, sy, padded[rows, iy, ix + 1], padded[rows, iy + 2, ix + 1]),
                            (ix, sx, padded[rows, iy + 1, ix], padded[rows, iy + 1, ix + 2])):
        if size == 1:
            offsets.append(torch.zeros_like(s0))
            continue
        edge = refine & ((i == 0) | (i == size - 1))
        second = (lo - 2.0 * s0) + hi
        flat = refine & ~edge & ~(second < 0)          # a NaN neighbour makes the comparison false
        offset = (0.5 * (lo - hi) / second).clamp(-0.5, 0.5)
        offsets.append(torch.where(refine & ~edge & ~flat, offset, torch.zeros_like(offset)))
        status = status | torch.where(edge, EDGE, 0) | torch.where(flat, FLAT, 0)
    integer = torch.stack([iy - sy // 2, ix - sx // 2], dim=1)
    integer = torch.where(found[:, None], integer, torch.zeros_like(integer))
    shift = integer.double() + torch.stack(offsets, dim=1)
    score = torch.where(found, s0, torch.full_like(s0, nan))
    if combine == 'shared':
        shift, integer, score, status = shift[0], integer[0], score[0], status[0]
    return {'shift': shift, 'integer': integer, 'score': score, 'status': status}


def coalign(image: torch.Tensor, template: torch.Tensor, max_shift=8, bad_image=None, bad_template=None, measure: str = 'zncc',
            min_overlap: float = 0.5, combine: str = 'shared') -> dict:
    """:func:`shift_sums`, :func:`scores_from_sums` and :func:`peak` in one call: the dict of :func:`peak` plus ``scores``
    [C, Sy, Sx] and ``sums`` [C, Sy, Sx, 6].  ``shift = (dy, dx)`` says that the image's content sits ``dy`` rows and ``dx``
    columns further along than the template's: ``shifted_grid(grid, dy, dx)`` is then the grid under which the image's pixels
    have the angles the template assigns to that content.  A template that is an exact whole-pixel copy of the image scores the
    measure's bound and gives that whole-pixel shift exactly (:func:`peak`: ``bound``).  Everything stays on the device; nothing
    waits for it."""
    if measure not in MEASURES:
        raise ValueError(f"measure must be 'zncc' or 'ssd', got {measure!r}")
    if combine not in ('shared', 'planes'):
        raise ValueError(f"combine must be 'shared' or 'planes', got {combine!r}")
    sums = shift_sums(image, template, max_shift, bad_image, bad_template)
    scores = scores_from_sums(sums, measure, min_overlap)
    out = peak(scores, combine, BOUNDS[measure])
    out.update(scores=scores, sums=sums)
    return out


def shifted_grid(grid: dict, dy: float, dx: float) -> dict:
    """The plate-scale dict of ``sunerf.evaluation.loader`` with ``crpix`` moved by ``(dx, dy)`` and everything else kept: pixel
    ``(r + dy, c + dx)`` of the new grid has the angles that pixel ``(r, c)`` had in the old one.  ``linear_plate_scale_axes``
    gives column ``c`` (counted from 1) the angle ``(c - crpix_x) cdelt_x + crval_x``, so ``crpix_x + dx`` does that, whatever the
    sign of ``cdelt``; a missing ``crpix`` is the frame's centre, as there."""
    h, w = grid['shape']
    cpx, cpy = grid.get('crpix', ((w + 1) / 2., (h + 1) / 2.))
    out = dict(grid)
    out['crpix'] = (cpx + float(dx), cpy + float(dy))
    return out
