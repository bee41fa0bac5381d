"""Link-level bit errors: what a channel estimate is worth to the receiver that uses it.

Every comparison of estimators here ends in channel MSE.  A receiver uses the estimate to equalise data symbols, so the first question
about an MSE gain is how many bit errors it removes, at which modulation order and SNR.  This module DEFINES the link: data symbols
through the TRUE channel plus noise, a one-tap equaliser that uses the ESTIMATE, a hard demapper and a bit-error count, as a pure
function of the frame's key, its noise scale, its true channel and the estimate:

* ``link_errors_host`` evaluates the definition in float64 with NumPy -- the CPU path and the yardstick;
* ``aft_link_errors_f32`` (csrc/k_link.hip, through ``hip_ops.LinkPlan``) evaluates it in float32 on the device, one launch per batch;
* ``LinkAccumulator`` sums a sweep's counts the way ``metrics.MseAccumulator`` sums squared errors; ``evaluation.get_link_stats`` is the
  sweep.

The definition.  For a frame: key ``kf`` (64 bits; for simulated frames ``chansim.frame_keys(seed, g)``, the simulator's own), true channel
``H`` and estimate ``E`` (complex64 ``[S, T]``), noise scale ``sigma`` (float32), ``m`` bits per symbol in {2, 4, 6, 8} (square QAM),
``L = 2^(m/2)`` levels per axis, ``d = sqrt(3 / (2 (L^2 - 1)))`` (unit mean symbol energy).  Over every grid element ``(s, t)`` that is
not a pilot position (``pilot_scs x pilot_symbols`` of the ``ChannelSimConfig``), ``q = s T + t``::

    word(stream, q) = splitmix64(kf ^ (stream << 32 | q))       streams 5 data bits, 6 data-noise radius, 7 data-noise angle
    w  = word(5, q) >> (64 - m),   gi = w >> (m/2),   gq = w & (L - 1)            the sent Gray codes of the I and the Q axis
    k  : k ^ (k >> 1) = g                                                          the level index of a Gray code
    x  = d ((2 ki - (L-1)) + j (2 kq - (L-1)))                                     the sent symbol
    y  = H[s,t] x + sigma sqrt(-ln u1) exp(j 2 pi u2)                              u = ((word >> 41) + 0.5) 2^-23 of streams 6 and 7
    c  = y conj(E[s,t]),   p = |E[s,t]|^2
    k^ = #{b in 1 .. L-1 : comp >= beta_b p},   beta_b = 2 d (b - L/2)             per axis, comp = Re c for I and Im c for Q
    bit errors    = sum popcount(gi ^ g^i) + popcount(gq ^ g^q),   g^ = k^ ^ (k^ >> 1)
    symbol errors = the number of elements with any bit wrong

This is zero-forcing with a hard decision and without a division: a total function with no special case for ``p = 0``.  The noise is the
simulator's Box-Muller (the angle is formed in turns and reduced before its sine and cosine); streams 0-4 stay the simulator's.  A frame
carries ``m (S T - Ps Pt)`` bits.  ``sigma`` for a frame at ``snr_db`` is ``float32(10^(-snr_db / 20))``, formed in double and rounded
once (``noise_sigma``; the rule of ``ChannelSimConfig.tables()["noise_sigma"]``).

The margin, which is what a float32 evaluation is compared through: for each (element, axis, boundary)
``|comp - beta_b p| / ((|H||x| + |noise|) |E| + |beta_b| p)``, 0 where the denominator is 0.  An (element, axis) is FLAGGED at ``tau``
when any of its boundaries has margin <= ``tau``: there a relative error of ``tau`` in the two sides may move the decision across that
boundary.  Because of the Gray map a flagged (element, axis) changes a frame's bit-error count by at most 1, and a
flagged element its symbol-error count by at most 1.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _abi
from .chansim import STREAM_DATA_BITS, STREAM_DATA_NOISE_ANGLE, STREAM_DATA_NOISE_RADIUS, ChannelSimConfig, frame_keys, words
from .synth import _splitmix64

BITS_PER_SYMBOL = (2, 4, 6, 8)
_POPCOUNT = np.array([bin(i).count("1") for i in range(16)], dtype=np.int64)


@dataclass(frozen=True)
class LinkConfig:
    """The link a frame's errors are counted on: the simulator's grid and pilot positions, and the modulation order."""
    sim: ChannelSimConfig = field(default_factory=ChannelSimConfig)
    bits_per_symbol: int = 4

    def __post_init__(self) -> None:
        if not isinstance(self.sim, ChannelSimConfig):
            raise ValueError(f"LinkConfig needs a chansim.ChannelSimConfig (got {type(self.sim).__name__})")
        m = self.bits_per_symbol
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in BITS_PER_SYMBOL:
            raise ValueError(f"bits_per_symbol = {m!r}: square QAM with one of {BITS_PER_SYMBOL} bits per symbol")
        object.__setattr__(self, "bits_per_symbol", int(m))
        S, T = self.sim.ofdm
        if S * T > 1 << 31:
            raise ValueError(f"ofdm grid {S} x {T}: the element index of the hash is 32 bits, at most 2^31 elements")

    @property
    def levels(self) -> int:
        return 1 << (self.bits_per_symbol // 2)

    @property
    def d(self) -> float:
        """Half the distance between neighbouring levels, for unit mean symbol energy."""
        return float(np.sqrt(3.0 / (2.0 * (self.levels ** 2 - 1.0))))

    @property
    def data_mask(self) -> np.ndarray:
        """bool ``[S, T]``: True where the grid carries data (everywhere but ``pilot_scs x pilot_symbols``)."""
        mask = np.ones(self.sim.ofdm, dtype=bool)
        mask[np.asarray(self.sim.pilot_scs)[:, None], np.asarray(self.sim.pilot_symbols)[None, :]] = False
        return mask

    @property
    def data_elements(self) -> int:
        return self.sim.ofdm[0] * self.sim.ofdm[1] - self.sim.pilot[0] * self.sim.pilot[1]

    @property
    def bits_per_frame(self) -> int:
        return self.bits_per_symbol * self.data_elements

    def to_struct(self) -> "_abi.AftLink":
        p = self.sim.fill_grid(_abi.AftLink())
        p.bits_per_symbol = self.bits_per_symbol
        return p


def noise_sigma(snr_db) -> np.ndarray:
    """``float32(10^(-snr_db / 20))``: formed in double, rounded once."""
    return (10.0 ** (-np.asarray(snr_db, dtype=np.float64) / 20.0)).astype(np.float32)


def gray_level(g) -> np.ndarray:
    """The level index ``k`` of a Gray code of at most four bits: ``k ^ (k >> 1) = g``."""
    g = np.asarray(g, dtype=np.int64)
    g = g ^ (g >> 1)
    return g ^ (g >> 2)


def constellation(bits_per_symbol: int) -> np.ndarray:
    """complex128 ``[2^m]``: the symbol every m-bit word ``w`` is sent as."""
    cfg = LinkConfig(bits_per_symbol=bits_per_symbol)
    m, L = cfg.bits_per_symbol, cfg.levels
    w = np.arange(1 << m)
    ki, kq = gray_level(w >> (m // 2)), gray_level(w & (L - 1))
    return cfg.d * ((2 * ki - (L - 1)) + 1j * (2 * kq - (L - 1)))


def _uniform(keys: np.ndarray, stream: int, q: np.ndarray) -> np.ndarray:
    return ((words(keys, stream, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23


def link_errors_host(cfg: LinkConfig, keys, ideal, est, sigma, tau: Optional[float] = None):
    """The definition in float64 on the given arrays: ``keys`` uint64 ``[n]`` (an int64 array is taken bit for bit), ``ideal`` / ``est``
    complex ``[n, S, T]``, ``sigma`` ``[n]`` -> ``counts`` int64 ``[n, 2]`` = (bit errors, symbol errors) per frame.  With ``tau``:
    ``(counts, errors, flags)``, ``errors`` int64 ``[n, S, T]`` the wrong bits of each element (0 at the pilots) and ``flags`` bool
    ``[n, S, T, 2]`` the flagged (element, axis) pairs at ``tau`` (module docstring; False at the pilots).  Needs no library."""
    keys = np.ascontiguousarray(keys)
    if keys.dtype == np.int64:
        keys = keys.view(np.uint64)
    if keys.dtype != np.uint64 or keys.ndim != 1:
        raise ValueError("keys must be a vector of 64-bit words (uint64, or int64 taken bit for bit)")
    n, (S, T) = len(keys), cfg.sim.ofdm
    H, E = np.asarray(ideal).astype(np.complex128), np.asarray(est).astype(np.complex128)
    if H.shape != (n, S, T) or E.shape != (n, S, T):
        raise ValueError(f"Expected ideal and est of shape ({n}, {S}, {T}), got {H.shape} and {E.shape}")
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if sigma.shape != (n,):
        raise ValueError(f"sigma must hold one value per frame ({n}), got {sigma.size}")
    m, L, d = cfg.bits_per_symbol, cfg.levels, cfg.d
    half = m // 2
    q = np.arange(S * T, dtype=np.uint64).reshape(1, S, T)
    kk = keys[:, None, None]
    w = (words(kk, STREAM_DATA_BITS, q) >> np.uint64(64 - m)).astype(np.int64)
    gi, gq = w >> half, w & (L - 1)
    x = d * ((2 * gray_level(gi) - (L - 1)) + 1j * (2 * gray_level(gq) - (L - 1)))
    u1, u2 = _uniform(kk, STREAM_DATA_NOISE_RADIUS, q), _uniform(kk, STREAM_DATA_NOISE_ANGLE, q)
    noise = sigma[:, None, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)
    c = (H * x + noise) * E.conj()
    p = E.real ** 2 + E.imag ** 2
    mask = cfg.data_mask[None]
    if tau is not None:
        reach = (np.abs(H) * np.abs(x) + np.abs(noise)) * np.abs(E)
        flags = np.zeros((n, S, T, 2), dtype=bool)
    wrong = np.zeros((n, S, T), dtype=np.int64)
    for axis, (comp, sent) in enumerate(((c.real, gi), (c.imag, gq))):
        level = np.zeros((n, S, T), dtype=np.int64)
        for b in range(1, L):
            beta = 2.0 * d * (b - L / 2)
            level += comp >= beta * p
            if tau is not None:
                den = reach + abs(beta) * p
                margin = np.divide(np.abs(comp - beta * p), den, out=np.zeros_like(den), where=den > 0)
                flags[..., axis] |= margin <= tau
        wrong += _POPCOUNT[sent ^ level ^ (level >> 1)]
    wrong *= mask
    counts = np.stack([wrong.sum(axis=(1, 2)), (wrong > 0).sum(axis=(1, 2))], axis=1).astype(np.int64)
    if tau is None:
        return counts
    flags &= mask[..., None]
    return counts, wrong, flags


# ---- the frame keys with torch ops, for frame numbers that live on the device (no synchronisation) ----

def _s64(v: int) -> int:
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _lsr(x: torch.Tensor, k: int) -> torch.Tensor:
    return (x >> k) & ((1 << (64 - k)) - 1)


def _splitmix64_torch(x: torch.Tensor) -> torch.Tensor:
    """``synth._splitmix64`` on an int64 tensor taken as 64-bit words (two's-complement arithmetic wraps as the unsigned one does)."""
    x = x + _s64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _s64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _s64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def frame_keys_torch(seed: int, frame_ids: torch.Tensor) -> torch.Tensor:
    """``chansim.frame_keys`` for an integer tensor of frame numbers, on its device: int64 ``[n]`` holding the keys' bits."""
    sk = int(_splitmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0])
    return _splitmix64_torch(frame_ids.reshape(-1).to(torch.int64) ^ _s64(sk))


class LinkAccumulator:
    """Bit and symbol errors of a sweep, with the surface of ``metrics.MseAccumulator``: ``update`` per batch, ``result`` once.

    ``update(est, ideal, meta)`` takes the frames' numbers from ``meta[0]`` (the loaders' ``file_no``: float32 as the reference's, so
    exact below 2^24; ``frame_ids=`` gives exact ones) and their SNR from ``meta[1]`` (``snr_db=`` overrides; one value or one per
    frame); the frame's key is ``chansim.frame_keys(seed, g)``.  ``est=None`` is perfect channel knowledge (``est = ideal``).  On a HIP
    device a batch is one launch of ``aft_link_errors_f32`` plus one small integer add into an int64 ``[2]`` device tensor: frame
    numbers and SNRs that are host tensors are hashed on the host and copied from pinned memory, device tensors are hashed with
    torch ops -- nothing synchronises.  On a CPU device the float64 definition runs.  ``result`` / ``result_ser`` close the sweep with
    one read and, with several ranks, the same 16-byte all-gather as the MSE accumulator."""

    def __init__(self, cfg: LinkConfig, device, seed: int = 0) -> None:
        if not isinstance(cfg, LinkConfig):
            raise ValueError(f"LinkAccumulator needs a LinkConfig (got {type(cfg).__name__})")
        self.cfg, self.seed = cfg, int(seed)
        self.device = torch.device(device)
        self._plan = None
        if self.device.type == "cuda":
            from .hip_ops import LinkPlan          # loads the extension: a missing .so raises here, loudly
            self._plan = LinkPlan(cfg, self.device)
            self.device = self._plan.device
        self.errors = torch.zeros(2, dtype=torch.int64, device=self.device)     # bit errors, symbol errors
        self.frames = 0

    def _stage(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(a).pin_memory().to(self.device, non_blocking=True)

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        S, T = self.cfg.sim.ofdm
        if ideal.dim() != 3 or tuple(ideal.shape[1:]) != (S, T) or ideal.dtype != torch.complex64:
            raise ValueError(f"ideal must be complex64 [B, {S}, {T}], got {ideal.dtype} {tuple(ideal.shape)}")
        if est is not None and (est.shape != ideal.shape or est.dtype != torch.complex64):
            raise ValueError(f"est must be complex64 {tuple(ideal.shape)} like ideal, got {est.dtype} {tuple(est.shape)}")
        b = ideal.shape[0]
        if frame_ids is None:
            if meta is None:
                raise ValueError("the frame numbers are needed: meta (file_no first) or frame_ids=")
            frame_ids = meta[0]
        if snr_db is None:
            if meta is None:
                raise ValueError("the SNR is needed: meta (snr second) or snr_db=")
            snr_db = meta[1]
        if b == 0:
            return
        on_device = lambda v: torch.is_tensor(v) and v.device.type == "cuda"  # noqa: E731
        host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)  # noqa: E731
        if self._plan is None or not on_device(frame_ids):
            g = np.rint(host(frame_ids).reshape(-1).astype(np.float64)).astype(np.int64)
            if g.size != b:
                raise ValueError(f"one frame number per frame ({b}), got {g.size}")
            keys = frame_keys(self.seed, g).view(np.int64)
        if self._plan is None or not on_device(snr_db):
            snr = host(snr_db).reshape(-1)
            if snr.size not in (1, b):
                raise ValueError(f"one SNR, or one per frame ({b}), got {snr.size}")
            sigma = noise_sigma(np.broadcast_to(snr, (b,)))
        if self._plan is None:
            H = ideal.detach().cpu().numpy()
            E = H if est is None else est.detach().cpu().numpy()
            self.errors += torch.from_numpy(link_errors_host(self.cfg, keys, H, E, sigma).sum(axis=0))
            self.frames += b
            return
        dev = self.device
        if on_device(frame_ids):
            if frame_ids.numel() != b:
                raise ValueError(f"one frame number per frame ({b}), got {frame_ids.numel()}")
            ids = frame_ids.reshape(-1).to(dev)
            keys_t = frame_keys_torch(self.seed, ids if not ids.is_floating_point() else ids.round())
        else:
            keys_t = self._stage(keys)
        if on_device(snr_db):
            if snr_db.numel() not in (1, b):
                raise ValueError(f"one SNR, or one per frame ({b}), got {snr_db.numel()}")
            sigma_t = torch.pow(10.0, -snr_db.reshape(-1).to(device=dev, dtype=torch.float64) / 20.0).to(torch.float32).expand(b).contiguous()
        else:
            sigma_t = self._stage(sigma)
        H = ideal.to(dev).contiguous()
        E = H if est is None else est.to(dev).contiguous()
        if torch.cuda.current_device() != dev.index:                # the launch belongs to the accumulator's device
            with torch.cuda.device(dev):
                counts = self._plan(H, E, keys_t, sigma_t)
        else:
            counts = self._plan(H, E, keys_t, sigma_t)
        self.errors += counts.sum(dim=0, dtype=torch.int64)
        self.frames += b

    def local_pair(self, which: int = 0) -> torch.Tensor:
        """float64 ``[2]`` on the device: (bit errors, bits sent) -- with ``which=1`` (symbol errors, symbols sent).  Exact below 2^53."""
        sent = self.frames * (self.cfg.bits_per_frame if which == 0 else self.cfg.data_elements)
        return torch.stack([self.errors[which].to(torch.float64), torch.tensor(float(sent), dtype=torch.float64, device=self.device)])

    def _rate(self, which: int, group) -> float:
        pair = self.local_pair(which)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():   # world_size 1 included: same code path on every launch
            gathered = [torch.empty_like(pair) for _ in range(dist.get_world_size(group))]
            dist.all_gather(gathered, pair, group=group)
            pair = torch.stack(gathered).sum(dim=0)
        errors, sent = pair.tolist()                         # the sweep's one read
        return errors / sent if sent > 0 else 0.0

    def result(self, group: Optional["torch.distributed.ProcessGroup"] = None) -> float:
        """Global bit-error rate over all ranks (integers summed: identical on every rank, whatever the order)."""
        return self._rate(0, group)

    def result_ser(self, group=None) -> float:
        """Global symbol-error rate."""
        return self._rate(1, group)
