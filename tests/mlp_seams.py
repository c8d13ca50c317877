"""Where the MLP kernels cut a batch: the 32-sample chunks that sit on a boundary of the work each kernel hands out.

A chunk is 32 consecutive samples of one ray, numbered ray-major: chunk id = ray * ceil(S / 32) + c (the stash layout,
csrc/sunerf_common.h:89-111).  Each rule below restates the source lines it cites and returns {chunk id: why}.
tests/test_mlp_seams_host.py holds the restatements to the sizes the C ABI exposes and to ops.wgrad_split;
tests/test_gpu_mlp_seams.py puts a float64-checked backward probe on the chunks listed here.  Plain helpers, imported by name."""

CHUNK = 32
ENC_FRAGS = 6                         # sunerf_common.h:44  SUNERF_KS0: encoding fragments of a stash chunk
FWD_RAYS_PER_WG = 4                   # weight_ring.h:8  WAVES: render_fwd.hip and render_bwd.hip:215 take one ray per wave
PIPE_RING = 16                        # bwd_pipe.hip:53  RING: chunk slots of a hand-off ring
PIPE_D, PIPE_PT = 256, 8              # bwd_pipe.hip:48  the pipelined backward's width and workspace tiles
PIPE_SLOT = (PIPE_D // 16) * 1024     # bwd_pipe.hip:57  SLOT: one chunk of dZ
STASH_FP16, STASH_PHASE = 0, 1        # include/sunerf_hip.h:111-112
MAX_FWD_GRID = 1024                   # render_fwd.hip:1177


def chunks_per_ray(S):
    return (S + CHUNK - 1) // CHUNK


def total_chunks(n_rays, S):
    return n_rays * chunks_per_ray(S)


def samples_of(chunk, S):
    """(ray, first sample, end sample) of a chunk."""
    ray, c = divmod(chunk, chunks_per_ray(S))
    return ray, CHUNK * c, min(CHUNK * c + CHUNK, S)


def ranges(total, parts):
    """[(first, end)] of the non-empty ones of `parts` contiguous ranges of ceil(total / parts) chunks (the last one short)."""
    per = -(-total // parts)
    return [(p * per, min(total, (p + 1) * per)) for p in range(parts) if p * per < total]


# ---- sizes: what the C ABI exposes ------------------------------------------------------------------------------------

def act_chunk_bytes(D, n_linear, fmt):
    """StashLayout::chunk_bytes (sunerf_common.h:107): 6 encoding fragments, then per activation layer D/16 fragments of
    16-bit phases or 2 x D/16 of fp16 sin + cos, 1 KiB each."""
    return ENC_FRAGS * 1024 + (n_linear - 1) * (1 if fmt == STASH_PHASE else 2) * (D // 16) * 1024


def act_stash_bytes(n_rays, S, D, n_linear, fmt):
    """sunerf_act_stash_bytes (render_fwd.hip:1220-1225): every chunk plus one spare; phases at D = 256 only."""
    if fmt == STASH_PHASE and D != PIPE_D:
        return 0
    return (total_chunks(n_rays, S) + 1) * act_chunk_bytes(D, n_linear, fmt)


def dz_chunk_bytes(D, n_linear):
    """render_bwd.hip:281: D/16 fp16 dZ fragments per activation layer."""
    return (n_linear - 1) * (D // 16) * 1024


def dz_stash_bytes(n_rays, S, D, n_linear):
    """sunerf_dz_stash_bytes (render_bwd.hip:611-615): every chunk plus the spare."""
    return (total_chunks(n_rays, S) + 1) * dz_chunk_bytes(D, n_linear)


def wgrad_split(n_linear, cus, D):
    """ops.wgrad_split (ops.py:496-501): n_linear x split (x 4 blocks at D = 512) workgroups fit the chip in one wave."""
    return max(1, cus // (n_linear * (4 if D > 256 else 1)))


def pipe_pipelines(n_linear, cus=256):
    """PipeLayout (bwd_pipe.hip:1083-1084): 8 XCD classes x the whole pipelines of 2 (n_linear - 1) workgroups a class holds."""
    return 8 * ((cus // 8) // (2 * (n_linear - 1)))


def pipe_workspace_bytes(n_rays, S, n_linear, cus=256):
    """sunerf_bwd_pipe_workspace_bytes = PipeLayout::total (bwd_pipe.hip:1076-1096, :1119-1124)."""
    def up(v):
        return (v + 255) // 256 * 256
    n_act, NP = n_linear - 1, pipe_pipelines(n_linear, cus)
    n_links = n_act - 1
    return (256 + up(cus * 64 * 4) + up((64 + NP * n_links * 4 * 32) * 4)
            + up(NP * n_links * PIPE_RING * PIPE_SLOT + cus * 4 * 2048) + up(max(total_chunks(n_rays, S), 1) * PIPE_SLOT)
            + up(n_act * NP * PIPE_PT * (PIPE_PT + 1) * 1024 * 4) + up(cus * (PIPE_PT + 2) * 1024 * 4))


def exact_chunk_samples(D):
    """chunk_samples (bwd_exact.hip:296): samples per chunk of the any-size fp32 backward."""
    return 16384 if D > 256 else 32768


# ---- seams: {chunk id: why} -------------------------------------------------------------------------------------------

def chunk_seams(n_rays, S):
    """The first and the last chunk of the batch; the last chunk of the first and of the last ray -- partial when S % 32 != 0,
    and with an odd chunk count per ray the one whose dgrad partner is the spare chunk (render_fwd.hip:1223)."""
    cpr, total = chunks_per_ray(S), total_chunks(n_rays, S)
    tail = ('partial ' if S % CHUNK else '') + 'last chunk of a ray' + (' (partner: the spare)' if cpr % 2 else '')
    seams = {cpr - 1: tail + ', first ray', total - 1: tail + ', last ray'}
    seams[0] = 'first chunk of the batch'
    return seams


def forward_seam_rays(n_rays, grid):
    """render_fwd.hip:898-907 and :1175-1179: workgroup g takes groups of 4 rays g, g + grid, ... with grid = min(groups, CUs or
    SUNERF_GRID_CAP_FWD, 1024): the last ray of a sweep, the first ray of every further sweep, the first ray of the last (partial)
    group.  The stash slices those rays write are what the backward reads (render_fwd.hip:934)."""
    groups = -(-n_rays // FWD_RAYS_PER_WG)
    grid = min(groups, grid, MAX_FWD_GRID)
    rays = {}
    for g in range(grid, groups, grid):
        rays[FWD_RAYS_PER_WG * g - 1] = f'last ray of forward sweep {g // grid - 1}'
        rays[FWD_RAYS_PER_WG * g] = f'first ray of forward sweep {g // grid}'
    rays[FWD_RAYS_PER_WG * (groups - 1)] = 'first ray of the last forward group' + (' (partial)' if n_rays % FWD_RAYS_PER_WG else '')
    return rays


def forward_seams(n_rays, S, grid):
    """The first and the last chunk of every ray of :func:`forward_seam_rays`."""
    cpr = chunks_per_ray(S)
    seams = {}
    for ray, why in forward_seam_rays(n_rays, grid).items():
        seams[ray * cpr] = why + ', first chunk'
        seams[ray * cpr + cpr - 1] = why + ', last chunk'
    return seams


def dgrad_seams(n_rays, S, grid):
    """render_bwd.hip:275-316: one ray per wave, its chunks in pairs (2 pr, 2 pr + 1); with an odd chunk count the last chunk's
    partner is the spare (:284, :306-316).  Workgroups of 4 rays over min(groups, CUs or SUNERF_GRID_CAP_DGRAD) (:658-661, :245)."""
    cpr = chunks_per_ray(S)
    seams = {}
    for ray in (0, n_rays - 1):
        base = ray * cpr
        for c in range(min(cpr, 4)):
            seams[base + c] = f'dgrad pair {c // 2}, {"second" if c % 2 else "first"} chunk'
        seams[base + cpr - 1] = 'dgrad last pair, ' + ('alone with the spare' if cpr % 2 else 'second chunk')
    for c, why in forward_seams(n_rays, S, grid).items():
        seams.setdefault(c, 'dgrad ' + why)
    return seams


def wgrad_seams(n_rays, S, split):
    """wgrad.hip:82-84: partial sum s of a layer covers chunks [s per, min(total, (s + 1) per)), per = ceil(total / split)."""
    seams = {}
    for s, (b, e) in enumerate(ranges(total_chunks(n_rays, S), split)):
        seams[b] = f'wgrad slice {s}/{split} first chunk'
        seams[e - 1] = f'wgrad slice {s}/{split} last chunk'
    return seams


def pipe_seams(n_rays, S, n_linear, cus=256, prologue_every=False):
    """bwd_pipe.hip:913-918: pipeline P takes chunks [P per, min(total, (P + 1) per)), per = ceil(total / NP): its first and last
    chunk, where its hand-off rings wrap (cbeg + 16 k, RING slots, :53, :531-532: the first two wraps and the last), the
    short last range.  The prologue (:942-946) splits the chunks over its `cus` workgroups the same way: the first and last chunk
    of the first two, a middle and the last non-empty workgroup's range (``prologue_every``: of all of them)."""
    seams = {}
    for P, (b, e) in enumerate(ranges(total_chunks(n_rays, S), pipe_pipelines(n_linear, cus))):
        seams[b] = f'pipeline {P} first chunk'
        seams[e - 1] = f'pipeline {P} last chunk'
        wraps = list(range(b + PIPE_RING, e, PIPE_RING))
        for k, c in enumerate(wraps):
            if k < 2 or k == len(wraps) - 1:
                seams[c] = f'pipeline {P} ring wrap {k + 1}'
    pro = ranges(total_chunks(n_rays, S), cus)
    keep = range(len(pro)) if prologue_every else sorted({0, 1, len(pro) // 2, len(pro) - 1} & set(range(len(pro))))
    for w in keep:
        b, e = pro[w]
        seams.setdefault(b, f'prologue workgroup {w} first chunk')
        seams.setdefault(e - 1, f'prologue workgroup {w} last chunk')
    return seams


def exact_seams(n_rays, S, D):
    """bwd_exact.hip:296 and :646-648: the any-size fp32 backward runs over the samples (ray-major) in chunks of C =
    chunk_samples(D); a ray whose samples straddle k C is split over two of them.  The 32-sample chunks holding samples k C - 1
    and k C."""
    C, seams = exact_chunk_samples(D), {}
    for k in range(1, -(-(n_rays * S) // C)):
        for g in (k * C - 1, k * C):
            ray, s = divmod(g, S)
            seams[ray * chunks_per_ray(S) + s // CHUNK] = f'fp32 chunk seam {k} (sample {g}: ray {ray}, sample {s})'
    return seams


def offset_seams(n_rays, S, D, n_linear, fmt, powers=(31, 32, 33, 34)):
    """The chunk whose activation-stash slice holds byte 2^k and the first chunk that starts at or past it: 32-bit offset
    arithmetic would wrap there."""
    return _offsets(total_chunks(n_rays, S), act_chunk_bytes(D, n_linear, fmt), 'stash', powers)


def dz_offset_seams(n_rays, S, D, n_linear, powers=(31, 32)):
    """The same for the dz stash of the two-kernel backward."""
    return _offsets(total_chunks(n_rays, S), dz_chunk_bytes(D, n_linear), 'dz stash', powers)


def _offsets(total, chunk_bytes, name, powers):
    seams = {}
    for k in powers:
        first = -(-(1 << k) // chunk_bytes)
        if first < total:
            seams[first] = f'{name} 2^{k}: first chunk at or past it'
            seams.setdefault(first - 1, f'{name} 2^{k}: chunk before it')
    return seams


def as_probes(seams, S):
    """[(ray, first sample, end sample, why)] of whole-chunk probes, in chunk order."""
    return [samples_of(c, S) + (f'chunk {c}: {why}',) for c, why in sorted(seams.items())]
