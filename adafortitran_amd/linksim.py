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

The soft link.  No OFDM system runs uncoded 64- or 256-QAM: what decides whether an MSE gain matters is how much soft information the
demapper hands the decoder.  The decoder-free measure of that is the bit-interleaved coded-modulation rate, the generalised mutual
information (GMI) of the LLRs.  ``link_llrs_host`` (float64), ``aft_link_soft_f32`` (csrc/k_link.hip, through ``hip_ops.LinkSoftPlan``),
``RateAccumulator`` and ``evaluation.get_link_rates`` are to it what the four names above are to the bit errors.  Per frame and data
element, with ``w, gi, gq, x, y, c, p`` exactly as above::

    levels   a_k = d (2k - (L-1)),  label g_k = k ^ (k >> 1),  k = 0 .. L-1
    metric   mu_k(comp) = a_k (a_k p - 2 comp)        |y - E x|^2 up to a constant, separable per axis, no division
    bit j of an axis's Gray code, MSB first:  bit_j(g) = (g >> (m/2 - 1 - j)) & 1
    Delta_j  = min{mu_k : bit_j(g_k) = 1} - min{mu_k : bit_j(g_k) = 0}
    LLR      Lambda_j = scale Delta_j                 positive favours bit 0; I-axis bits 0 .. m/2-1, Q-axis bits m/2 .. m-1 (the order of w)
    loss_f  += log2(1 + exp(-(1 - 2 b_j) factor_f Lambda_j))       b_j the sent bit, for each of the K factors

``scale`` is a float32 per frame (``llr_scale``: one over the noise variance plus the estimate's error variance), ``factors`` float32
``[K]``, 1 <= K <= 8.  The LLR at a pilot position is 0.  A frame's rate at factor f is ``m - loss_f / data_elements`` bit/symbol; it
may be negative (over-confident LLRs under a mismatched channel, which is why the loss is evaluated on a grid of factors in one pass),
and the best of the grid is the GMI's supremum over the LLR scale taken on that grid.

What a float32 evaluation of the LLRs is compared through: ``q = scale A (A p + 2 R)`` with ``A = (L-1) d`` the outermost level and
``R = (|H||x| + |noise|) |E|`` the reach of ``comp`` -- every ``|mu_k| <= A (A p + 2 R)``, so an evaluation whose metrics err by a
relative ``e`` of that errs in ``Lambda_j`` by about ``2 e q``.  The loss is monotone in every ``Lambda_j``, so the losses at
``Lambda -+ e_lambda q`` (each bit moved towards, or away from, the sent bit) are an exact interval for every evaluation whose LLRs
are within ``e_lambda q``.
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


def _front(cfg: LinkConfig, keys, ideal, est, sigma):
    """What the hard and the soft definition share, in float64: the checked operands and, per element, the sent Gray codes ``gi`` / ``gq``,
    ``c = y conj(E)``, ``p = |E|^2`` and the reach ``(|H||x| + |noise|) |E|`` of a component of ``c``."""
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
    q = np.arange(S * T, dtype=np.uint64).reshape(1, S, T)
    kk = keys[:, None, None]
    w = (words(kk, STREAM_DATA_BITS, q) >> np.uint64(64 - m)).astype(np.int64)
    gi, gq = w >> (m // 2), w & (L - 1)
    x = d * ((2 * gray_level(gi) - (L - 1)) + 1j * (2 * gray_level(gq) - (L - 1)))
    u1, u2 = _uniform(kk, STREAM_DATA_NOISE_RADIUS, q), _uniform(kk, STREAM_DATA_NOISE_ANGLE, q)
    noise = sigma[:, None, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)
    c = (H * x + noise) * E.conj()
    p = E.real ** 2 + E.imag ** 2
    reach = (np.abs(H) * np.abs(x) + np.abs(noise)) * np.abs(E)
    return gi, gq, c, p, reach


def link_errors_host(cfg: LinkConfig, keys, ideal, est, sigma, tau: Optional[float] = None):
    """The definition in float64 on the given arrays: ``keys`` uint64 ``[n]`` (an int64 array is taken bit for bit), ``ideal`` / ``est``
    complex ``[n, S, T]``, ``sigma`` ``[n]`` -> ``counts`` int64 ``[n, 2]`` = (bit errors, symbol errors) per frame.  With ``tau``:
    ``(counts, errors, flags)``, ``errors`` int64 ``[n, S, T]`` the wrong bits of each element (0 at the pilots) and ``flags`` bool
    ``[n, S, T, 2]`` the flagged (element, axis) pairs at ``tau`` (module docstring; False at the pilots).  Needs no library."""
    gi, gq, c, p, reach = _front(cfg, keys, ideal, est, sigma)
    (n, S, T), L, d = c.shape, cfg.levels, cfg.d
    mask = cfg.data_mask[None]
    if tau is not None:
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


DEFAULT_FACTORS = tuple(2.0 ** -k for k in range(8))        # 1, 1/2, ..., 1/128: the grid the GMI's supremum over the LLR scale is taken on
MAX_FACTORS = 8


def llr_scale(snr_db, err_var=0.0) -> np.ndarray:
    """``float32(1 / (10^(-snr_db / 10) + err_var))``: one over the noise variance plus the estimate's error variance, formed in double
    and rounded once."""
    return (1.0 / (10.0 ** (-np.asarray(snr_db, dtype=np.float64) / 10.0) + float(err_var))).astype(np.float32)


def _factors(factors) -> np.ndarray:
    f = np.asarray(factors, dtype=np.float32).reshape(-1)
    if not 1 <= f.size <= MAX_FACTORS:
        raise ValueError(f"between 1 and {MAX_FACTORS} factors, got {f.size}")
    return f


def link_llrs_host(cfg: LinkConfig, keys, ideal, est, sigma, scale, factors=(1.0,), e_lambda: Optional[float] = None):
    """The soft definition (module docstring) in float64: operands as ``link_errors_host``'s, ``scale`` ``[n]`` and ``factors`` ``[K]``
    taken as the float32 numbers they are -> ``(loss float64 [n, K], llr float64 [n, S, T, m])``, the LLRs 0 at the pilots.  With
    ``e_lambda``: ``(loss, llr, loss_lo, loss_hi, q)``, ``q [n, S, T, m] = scale A (A p + 2 R)`` (0 at the pilots) and ``loss_lo`` /
    ``loss_hi`` the losses at ``Lambda -+ e_lambda q``, every bit moved towards / away from the sent bit.  Needs no library."""
    gi, gq, c, p, reach = _front(cfg, keys, ideal, est, sigma)
    (n, S, T), m, L, d = c.shape, cfg.bits_per_symbol, cfg.levels, cfg.d
    half = m // 2
    scale = np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(-1)
    if scale.shape != (n,):
        raise ValueError(f"scale must hold one value per frame ({n}), got {scale.size}")
    factors = _factors(factors).astype(np.float64)
    k = np.arange(L)
    a, label = d * (2 * k - (L - 1)), k ^ (k >> 1)
    mask = cfg.data_mask[None, :, :, None]
    llr = np.empty((n, S, T, m))
    sign = np.empty((n, S, T, m))                              # 1 - 2 b_j
    for axis, (comp, sent) in enumerate(((c.real, gi), (c.imag, gq))):
        mu = a * (a * p[..., None] - 2.0 * comp[..., None])                      # [n, S, T, L]
        for j in range(half):
            one = ((label >> (half - 1 - j)) & 1).astype(bool)
            llr[..., axis * half + j] = mu[..., one].min(axis=-1) - mu[..., ~one].min(axis=-1)
            sign[..., axis * half + j] = 1 - 2 * ((sent >> (half - 1 - j)) & 1)
    llr *= scale[:, None, None, None] * mask

    def losses(lam):
        z = -(sign * lam)
        return np.stack([(np.logaddexp(0.0, f * z) * mask).sum(axis=(1, 2, 3)) for f in factors], axis=1) / np.log(2.0)

    loss = losses(llr)
    if e_lambda is None:
        return loss, llr
    A = (L - 1) * d
    q = np.broadcast_to((scale[:, None, None] * A * (A * p + 2.0 * reach))[..., None] * mask, llr.shape).copy()
    return loss, llr, losses(llr + sign * (e_lambda * q)), losses(llr - sign * (e_lambda * q)), q


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


class _FrameSweep:
    """What the accumulators of a sweep share: a batch's checked operands where the accumulator computes.  ``_operands`` returns None
    for an empty batch, else ``(b, H, E, keys, per_frame)``: on a CPU device NumPy arrays for the float64 definition, on a HIP device
    tensors for the plan -- frame numbers and SNRs that are host tensors are hashed and converted on the host and copied from pinned
    memory, device tensors with torch ops, so nothing synchronises.  ``per_frame`` holds one float32 ``[b]`` operand per entry of
    ``of_snr``, pairs ``(numpy function, torch function on a float64 tensor)`` of the SNR in dB."""

    def _open(self, cfg: LinkConfig, device, seed: int, plan_name: str) -> None:
        if not isinstance(cfg, LinkConfig):
            raise ValueError(f"{type(self).__name__} needs a LinkConfig (got {type(cfg).__name__})")
        self.cfg, self.seed = cfg, int(seed)
        self.device = torch.device(device)
        self._plan = None
        if self.device.type == "cuda":
            from . import hip_ops                  # loads the extension: a missing .so raises here, loudly
            self._plan = getattr(hip_ops, plan_name)(cfg, self.device)
            self.device = self._plan.device
        self.frames = 0

    def _stage(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(a).pin_memory().to(self.device, non_blocking=True)

    def _operands(self, est, ideal, meta, frame_ids, snr_db, of_snr):
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
            return None
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
            per_frame = [on_host(np.broadcast_to(snr, (b,))) for on_host, _ in of_snr]
        if self._plan is None:
            H = ideal.detach().cpu().numpy()
            return b, H, (H if est is None else est.detach().cpu().numpy()), keys, per_frame
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
            snr_t = snr_db.reshape(-1).to(device=dev, dtype=torch.float64)
            per_frame_t = [on_dev(snr_t).to(torch.float32).expand(b).contiguous() for _, on_dev in of_snr]
        else:
            per_frame_t = [self._stage(a) for a in per_frame]
        H = ideal.to(dev).contiguous()
        return b, H, (H if est is None else est.to(dev).contiguous()), keys_t, per_frame_t

    def _launch(self, *args, **kw):
        """The plan on the accumulator's device: the launch belongs to it, whichever device is current."""
        if torch.cuda.current_device() != self.device.index:
            with torch.cuda.device(self.device):
                return self._plan(*args, **kw)
        return self._plan(*args, **kw)

    @staticmethod
    def _all_ranks(local: torch.Tensor, group) -> list:
        """The sweep's one read: ``local`` (float64, on the device) summed over all ranks -- with several, one all-gather."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():   # world_size 1 included: same code path on every launch
            gathered = [torch.empty_like(local) for _ in range(dist.get_world_size(group))]
            dist.all_gather(gathered, local, group=group)
            local = torch.stack(gathered).sum(dim=0)
        return local.tolist()


_SIGMA_OF_SNR = (noise_sigma, lambda snr: torch.pow(10.0, -snr / 20.0))


class LinkAccumulator(_FrameSweep):
    """Bit and symbol errors of a sweep, with the surface of ``metrics.MseAccumulator``: ``update`` per batch, ``result`` once.

    ``update(est, ideal, meta)`` takes the frames' numbers from ``meta[0]`` (the loaders' ``file_no``: float32 as the reference's, so
    exact below 2^24; ``frame_ids=`` gives exact ones) and their SNR from ``meta[1]`` (``snr_db=`` overrides; one value or one per
    frame); the frame's key is ``chansim.frame_keys(seed, g)``.  ``est=None`` is perfect channel knowledge (``est = ideal``).  On a HIP
    device a batch is one launch of ``aft_link_errors_f32`` plus one small integer add into an int64 ``[2]`` device tensor: frame
    numbers and SNRs that are host tensors are hashed on the host and copied from pinned memory, device tensors are hashed with
    torch ops -- nothing synchronises.  On a CPU device the float64 definition runs.  ``result`` / ``result_ser`` close the sweep with
    one read and, with several ranks, the same 16-byte all-gather as the MSE accumulator."""

    def __init__(self, cfg: LinkConfig, device, seed: int = 0) -> None:
        self._open(cfg, device, seed, "LinkPlan")
        self.errors = torch.zeros(2, dtype=torch.int64, device=self.device)     # bit errors, symbol errors

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        ops = self._operands(est, ideal, meta, frame_ids, snr_db, (_SIGMA_OF_SNR,))
        if ops is None:
            return
        b, H, E, keys, (sigma,) = ops
        if self._plan is None:
            self.errors += torch.from_numpy(link_errors_host(self.cfg, keys, H, E, sigma).sum(axis=0))
        else:
            self.errors += self._launch(H, E, keys, sigma).sum(dim=0, dtype=torch.int64)
        self.frames += b

    def local_pair(self, which: int = 0) -> torch.Tensor:
        """float64 ``[2]`` on the device: (bit errors, bits sent) -- with ``which=1`` (symbol errors, symbols sent).  Exact below 2^53."""
        sent = self.frames * (self.cfg.bits_per_frame if which == 0 else self.cfg.data_elements)
        return torch.stack([self.errors[which].to(torch.float64), torch.tensor(float(sent), dtype=torch.float64, device=self.device)])

    def _rate(self, which: int, group) -> float:
        errors, sent = self._all_ranks(self.local_pair(which), group)
        return errors / sent if sent > 0 else 0.0

    def result(self, group: Optional["torch.distributed.ProcessGroup"] = None) -> float:
        """Global bit-error rate over all ranks (integers summed: identical on every rank, whatever the order)."""
        return self._rate(0, group)

    def result_ser(self, group=None) -> float:
        """Global symbol-error rate."""
        return self._rate(1, group)


class RateAccumulator(_FrameSweep):
    """The achievable rate of a sweep from its max-log LLRs (module docstring, "the soft link"), with ``LinkAccumulator``'s ``update``
    surface.  A frame's LLR scale is ``llr_scale(snr_db, err_var)``: ``err_var`` is what the caller knows of the estimate's error
    variance (0: the LLRs trust the estimate as if it were the channel), and ``factors`` the grid of further scale factors the loss is
    evaluated on in the same pass.  On a HIP device a batch is one launch of ``aft_link_soft_f32`` plus one float64 add into a device
    tensor ``[K]``; nothing synchronises.  On a CPU device the float64 definition runs.  ``result`` returns the K rates in bit/symbol
    (``m - loss / data elements``; a rate may be negative), ``result_gmi`` their maximum; either is one read and, with several ranks,
    one all-gather of ``K + 1`` float64 (the K losses and the frames).  The losses are float sums: ranks that split a sweep differently
    agree to rounding, not bit for bit -- every rank of one sweep reports the same number."""

    def __init__(self, cfg: LinkConfig, device, seed: int = 0, factors=(1.0,), err_var: float = 0.0) -> None:
        self._open(cfg, device, seed, "LinkSoftPlan")
        self.err_var = float(err_var)
        if not self.err_var >= 0.0:
            raise ValueError(f"err_var = {err_var!r}: a variance, at least 0")
        self.factors = _factors(factors)
        self.loss = torch.zeros(len(self.factors), dtype=torch.float64, device=self.device)
        self._factors_t = None if self._plan is None else torch.from_numpy(self.factors).to(self.device)
        self._of_snr = (_SIGMA_OF_SNR, (lambda snr: llr_scale(snr, self.err_var),
                                        lambda snr: 1.0 / (torch.pow(10.0, -snr / 10.0) + self.err_var)))

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        ops = self._operands(est, ideal, meta, frame_ids, snr_db, self._of_snr)
        if ops is None:
            return
        b, H, E, keys, (sigma, scale) = ops
        if self._plan is None:
            self.loss += torch.from_numpy(link_llrs_host(self.cfg, keys, H, E, sigma, scale, self.factors)[0].sum(axis=0))
        else:
            self.loss += self._launch(H, E, keys, sigma, scale, self._factors_t)[0].sum(dim=0, dtype=torch.float64)
        self.frames += b

    def result(self, group: Optional["torch.distributed.ProcessGroup"] = None) -> list:
        """The K rates in bit/symbol over all ranks, one per factor (0.0 each for an empty sweep)."""
        frames = torch.tensor([float(self.frames)], dtype=torch.float64, device=self.device)
        *loss, frames = self._all_ranks(torch.cat([self.loss, frames]), group)
        m, elements = self.cfg.bits_per_symbol, frames * self.cfg.data_elements
        return [m - v / elements if elements > 0 else 0.0 for v in loss]

    def result_gmi(self, group=None) -> float:
        """The best rate of the factor grid: the GMI's supremum over the LLR scale, taken on the grid."""
        return max(self.result(group))
