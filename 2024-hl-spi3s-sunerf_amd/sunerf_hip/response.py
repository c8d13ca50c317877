"""Response sets: the temperature responses of any instrument's channels for the density / temperature integral
(include/sunerf_hip_response.h, csrc/dt_response_set.hip).

A ``ResponseSet`` is M channels, each with a positive integer *code* (what a ray's ``wavelengths`` row carries: for AIA the
wavelength in Angstrom; a second instrument's 171 channel gets another code, e.g. 10171), a name, its own strictly increasing
log T grid and its response on it, exposure time or gain folded in.  Everything is validated here, on the host; the kernels trust
the arrays they are given.  Tables arrive as arrays: no instrument file format is parsed here except the AIA table the renderer
already reads (``sunerf_hip.genx``).
"""
import numpy as np
import torch

MAX_CHANNELS = 64
MAX_NODES = 4096
MAX_COLUMNS = 8
MAX_CODE = 1 << 24
LDS_LIMIT = 160 * 1024


class ResponseSet:
    """``ResponseSet([(code, name, logt, resp), ...])``.  Immutable after construction; picklable; ``.to(device)`` caches the four
    device arrays of the C ABI."""

    def __init__(self, channels):
        channels = list(channels)
        if not 1 <= len(channels) <= MAX_CHANNELS:
            raise ValueError(f'a response set has 1 .. {MAX_CHANNELS} channels, got {len(channels)}')
        codes, names, grids, resps = [], [], [], []
        for entry in channels:
            if len(entry) != 4:
                raise ValueError('every channel is (code, name, logt, resp)')
            code, name, logt, resp = entry
            try:
                ok = float(code) == int(code) and 0 < int(code) < MAX_CODE
            except (TypeError, ValueError, OverflowError):
                ok = False
            if not ok:
                raise ValueError(f'channel code {code!r} is not a positive integer below 2^24 (exact in fp32)')
            code = int(code)
            if code in codes:
                raise ValueError(f'channel code {code} occurs twice in the set')
            with np.errstate(over='ignore'):       # a value beyond fp32 becomes inf and is refused below
                logt = np.array(logt.detach().cpu().numpy() if torch.is_tensor(logt) else logt, dtype=np.float32)
                resp = np.array(resp.detach().cpu().numpy() if torch.is_tensor(resp) else resp, dtype=np.float32)
            if logt.ndim != 1 or resp.shape != logt.shape:
                raise ValueError(f'channel {code}: logt and resp must be 1-D arrays of one length, got {logt.shape} and {resp.shape}')
            if logt.size < 2:
                raise ValueError(f'channel {code}: a grid needs at least 2 nodes, got {logt.size}')
            if not (np.isfinite(logt).all() and np.isfinite(resp).all()):
                raise ValueError(f'channel {code}: the grid and the response must be finite (in fp32)')
            if not (np.diff(logt) > 0).all():
                raise ValueError(f'channel {code}: the log T grid must be strictly increasing (in fp32)')
            codes.append(code); names.append(str(name)); grids.append(logt); resps.append(resp)
        total = sum(g.size for g in grids)
        if total > MAX_NODES:
            raise ValueError(f'a response set holds at most {MAX_NODES} nodes in all, got {total}')
        self._codes = tuple(codes)
        self._names = tuple(names)
        self._offsets = np.concatenate([[0], np.cumsum([g.size for g in grids])]).astype(np.int32)
        self._logt = np.concatenate(grids)
        self._resp = np.concatenate(resps)
        self._device = {}

    # ---- constructors -----------------------------------------------------------------------------------------------------
    @classmethod
    def aia(cls, path_or_tables="sunerf/data/aia_temp_resp.genx", exposure=2.9):
        """The seven AIA channels as ``DensityTemperatureRadiativeTransfer`` holds them: ``path_or_tables`` is the ``.genx`` path or
        ``(logte [7, n], tresp [7, n])``; the response is ``tresp * exposure`` cast to fp32, the rendering's two buffers by bits."""
        from .genx import CHANNELS, read_aia_temp_resp
        logte, tresp = read_aia_temp_resp(path_or_tables) if isinstance(path_or_tables, str) else path_or_tables
        logte = torch.as_tensor(logte).float()
        resp = torch.as_tensor(tresp * exposure).float()
        if logte.shape != resp.shape or logte.ndim != 2 or logte.shape[0] != len(CHANNELS):
            raise ValueError(f'the AIA tables are ({len(CHANNELS)}, n) arrays, got {tuple(logte.shape)} and {tuple(resp.shape)}')
        return cls([(c, f'AIA {c}', logte[i], resp[i]) for i, c in enumerate(CHANNELS)])

    def concat(self, other, code_offset=0):
        """This set followed by ``other``'s channels, their codes raised by ``code_offset`` (a second instrument whose files use
        the wavelength as the code)."""
        return ResponseSet(self.channels() + [(c + int(code_offset), nm, x, y) for c, nm, x, y in other.channels()])

    # ---- what it holds ------------------------------------------------------------------------------------------------------
    def channels(self):
        return [(c, nm) + self.table(i) for i, (c, nm) in enumerate(zip(self._codes, self._names))]

    def table(self, row):
        """(logt, resp) fp32 arrays of channel ``row``."""
        a, b = int(self._offsets[row]), int(self._offsets[row + 1])
        return self._logt[a:b].copy(), self._resp[a:b].copy()

    @property
    def n_channels(self):
        return len(self._codes)

    @property
    def n_nodes(self):
        return int(self._offsets[-1])

    @property
    def codes(self):
        return self._codes

    @property
    def names(self):
        return self._names

    @property
    def keys(self):
        """``str(code)`` per channel: the names of the models' ``log_absortpion`` ParameterDict."""
        return tuple(str(c) for c in self._codes)

    @property
    def offsets(self):
        return self._offsets.copy()

    def __len__(self):
        return len(self._codes)

    def __repr__(self):
        return 'ResponseSet(' + ', '.join(f'{c}: {nm!r} [{self._offsets[i + 1] - self._offsets[i]}]'
                                          for i, (c, nm) in enumerate(zip(self._codes, self._names))) + ')'

    def __eq__(self, other):
        return (isinstance(other, ResponseSet) and self._codes == other._codes and self._names == other._names
                and np.array_equal(self._offsets, other._offsets) and np.array_equal(self._logt, other._logt)
                and np.array_equal(self._resp, other._resp))

    __hash__ = None

    def index_of(self, codes):
        """The set's row of every code of ``codes`` (a code or a sequence); an unknown code raises and names the known ones."""
        single = not hasattr(codes, '__iter__')
        rows = []
        for c in ([codes] if single else codes):
            try:
                ok = float(c) == int(c) and int(c) in self._codes
            except (TypeError, ValueError, OverflowError):
                ok = False
            if not ok:
                raise ValueError(f'code {c!r} is not a channel of the response set ({", ".join(self.keys)})')
            rows.append(self._codes.index(int(c)))
        return rows[0] if single else rows

    def check_codes(self, wavelengths):
        """Raises when ``wavelengths`` (any shape; entries <= 0 are absent columns) holds a positive code the set does not have
        -- such a column would render 0 and train nothing.  One host read: call it once per observation set, not per step."""
        values = torch.unique(torch.as_tensor(wavelengths).detach().float()).cpu().tolist()
        unknown = [v for v in values if v > 0 and not (v == int(v) and int(v) in self._codes)]
        if any(v != v for v in values):
            unknown.append(float('nan'))
        if unknown:
            raise ValueError(f'codes {unknown} are not channels of the response set ({", ".join(self.keys)})')

    def on_nodes(self, nodes):
        """(M, K) float64 torch tensor: every channel's response linearly interpolated on ``nodes`` (K,), 0 outside the channel's
        own grid (its extrap-0 rule)."""
        nodes = np.asarray(torch.as_tensor(nodes).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
        out = np.zeros((self.n_channels, nodes.size), dtype=np.float64)
        for i in range(self.n_channels):
            x, y = self.table(i)
            out[i] = np.interp(nodes, x.astype(np.float64), y.astype(np.float64), left=0., right=0.)
        return torch.from_numpy(out)

    def shared_grid(self):
        """The fp32 log T grid all channels share, or None when they differ."""
        first = self.table(0)[0]
        for i in range(1, self.n_channels):
            if not np.array_equal(self.table(i)[0], first):
                return None
        return first

    # ---- the kernels' limits -------------------------------------------------------------------------------------------------
    def bwd_lds_bytes(self, n_samples, n_wavelengths):
        """LDS bytes of the backward for this set (``sunerf_dt_response_bwd_lds_bytes``, restated: no library needed)."""
        return (200 + 2 * self.n_nodes + 8 * int(n_samples) * int(n_wavelengths)) * 4

    def fits(self, n_samples, n_wavelengths):
        return 1 <= n_wavelengths <= MAX_COLUMNS and n_samples >= 3 and self.bwd_lds_bytes(n_samples, n_wavelengths) <= LDS_LIMIT

    def max_samples(self, n_wavelengths):
        """The largest sample count per ray the backward takes at ``n_wavelengths`` columns."""
        return (LDS_LIMIT // 4 - 200 - 2 * self.n_nodes) // (8 * int(n_wavelengths))

    # ---- device arrays ---------------------------------------------------------------------------------------------------------
    def to(self, device):
        """(offsets int32 [M+1], codes fp32 [M], logt fp32 [n], resp fp32 [n]) on ``device``, made once per device."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        got = self._device.get(device)
        if got is None:
            got = (torch.from_numpy(self._offsets.copy()).to(device),
                   torch.tensor(self._codes, dtype=torch.float32, device=device),
                   torch.from_numpy(self._logt.copy()).to(device), torch.from_numpy(self._resp.copy()).to(device))
            self._device[device] = got
        return got

    # ---- persistence -----------------------------------------------------------------------------------------------------------
    def __getstate__(self):
        return {'codes': self._codes, 'names': self._names, 'offsets': self._offsets, 'logt': self._logt, 'resp': self._resp}

    def __setstate__(self, state):
        self._codes, self._names = tuple(state['codes']), tuple(state['names'])
        self._offsets, self._logt, self._resp = state['offsets'], state['logt'], state['resp']
        self._device = {}

    def save(self, path):
        """One ``.npz``: codes, names, offsets, logt, resp."""
        with open(path, 'wb') as fh:
            np.savez(fh, codes=np.array(self._codes, dtype=np.int64), names=np.array(self._names, dtype=str),
                     offsets=self._offsets, logt=self._logt, resp=self._resp)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            off = f['offsets']
            return cls([(int(c), str(nm), f['logt'][off[i]:off[i + 1]], f['resp'][off[i]:off[i + 1]])
                        for i, (c, nm) in enumerate(zip(f['codes'], f['names']))])


def as_response_set(channels):
    """``channels`` of a DT field class -> (codes tuple, ResponseSet or None): a ``ResponseSet`` or a sequence of codes."""
    if isinstance(channels, ResponseSet):
        return channels.codes, channels
    codes = []
    for c in channels:
        try:
            ok = float(c) == int(c) and 0 < int(c) < MAX_CODE
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok or int(c) in codes:
            raise ValueError(f'channels must be unique positive integer codes below 2^24, got {c!r}')
        codes.append(int(c))
    if not 1 <= len(codes) <= MAX_CHANNELS:
        raise ValueError(f'a model has 1 .. {MAX_CHANNELS} channels, got {len(codes)}')
    return tuple(codes), None
