"""A physical OFDM channel generator: training and evaluation data without a dataset.

The reference ships no data (its ``.mat`` files came from a MATLAB link-level simulation) and
``synth.make_inputs`` draws pilots and targets independently, which is fine for parity and timing and useless for learning.  This module
DEFINES a doubly-selective multipath Rayleigh channel over the OFDM grid, the noisy LS estimate at the pilot positions and the three
conditions the frame was drawn with, as a pure function of ``(seed, g)``, ``g`` the frame's global number:

* ``simulate_frames_host`` evaluates the definition in float64 with NumPy -- the CPU path and the yardstick;
* ``aft_channel_sim_f32`` (csrc/k_chansim.hip, through ``hip_ops.ChannelSimPlan``) evaluates it in float32 on the device, one launch
  per batch;
* ``SynthLoader`` yields ``ingest.ResidentLoader``'s batches from either; ``make_pack`` gives fixed sets in ``pack_mat_folder``'s format.

The model, for frame ``g`` (sum-of-sinusoids taps, ``M = rays``; ``T_sym`` the symbol period, ``df`` the subcarrier spacing)::

    h_p(t)  = amp_p * sum_m exp(j 2 pi (f_D T_sym cos(alpha_pm) t + phi_pm)),   alpha_pm = 2 pi (m + u_pm) / M,  phi_pm = 2 pi u'_pm
    H[s, t] = sum_p h_p(t) exp(-j 2 pi s df d_p DS)                             d_p the tap's normalised delay, DS the delay spread
    pilots  = H at the pilot positions + CN(0, 10^(-snr/10))                    Box-Muller on two uniforms (k + 0.5) 2^-23

with ``amp_p = sqrt(pw_p / sum(pw) / M)``, so ``E|H|^2 = 1``, ``E[H[s,t+k] conj H[s,t]] = J0(2 pi f_D k T_sym)`` (the angles of a tap
cover the circle uniformly) and ``E[H[s+d,t] conj H[s,t]] = sum_p pw_p exp(-j 2 pi d df d_p DS) / sum(pw)``.

Random words are counter-based on ``synth._splitmix64``: ``word(seed, g, stream, index) = sm(sm(sm(seed) ^ g) ^ (stream << 32 | index))``
with the streams below.  The configuration the definition sees is the one the device sees: the tables are rounded to float32 ONCE
(``ChannelSimConfig.tables``), the two spacing-times-condition products are formed in float64 and rounded to float32 once.

Antenna correlation: Kronecker frame groups.  ``antennas = (R, N)`` (receive antennas by transmit streams) makes every
``G = R N <= AFT_CHANSIM_MAX_GROUP = 16`` consecutive frames the antennas of ONE receiver: global frame ``g`` is member ``a = g % G`` of
group ``g // G``, ``a = r N + s`` -- the frame order the links' ``branches=`` (``r``) and ``streams=`` (``r 2 + s``) already group by.
``rx_correlation`` / ``tx_correlation`` give the R x R and N x N correlation matrices: ``None`` the identity, a real or complex scalar
``rho``, ``|rho| < 1``, the exponential model ``C[i][j] = rho^(i-j)`` for ``i >= j`` and its conjugate above the diagonal, or a
Hermitian positive-definite matrix with unit diagonal.  ``tables()["mix"]`` is ``L = kron(chol(C_rx), chol(C_tx))`` (lower Cholesky
factors, so ``L`` is lower triangular in the order ``a = r N + s``), formed in float64 and rounded to complex64 ONCE; the entries above
the diagonal are exact zeros, and with both correlations ``None`` it is the exact identity.  For frame ``g`` of a configuration with
``G > 1``, ``lead = G (g // G)``:

* conditions: the three condition indices are picked from the LEADER's key ``frame_keys(seed, lead)`` -- the members of a group share
  SNR, delay spread and Doppler (``frame_conditions``, ``SynthLoader``'s meta and ``make_pack`` follow);
* source gains: for ``j = 0 .. a``, ``z_j[p][t]`` is ``h_p(t)`` above (``amp_p`` included) from the angle and phase streams of the key
  of frame ``lead + j``, at the group's Doppler;
* mixing: ``h_a[p][t] = sum_{j <= a} L[a][j] z_j[p][t]``, in increasing ``j`` from ``+0``; on the device one complex term is two fused
  multiply-adds per component, the form of the pilot sum: ``re = fmaf(L.re, z.re, fmaf(-L.im, z.im, re))``,
  ``im = fmaf(L.re, z.im, fmaf(L.im, z.re, im))``;
* everything after that is the ungrouped frame's: the delay phasors and the sum over the taps at the group's delay spread, the pilot
  noise from frame ``g``'s OWN noise streams at the group's ``noise_sigma``;
* the frame's key stays ``frame_keys(seed, g)``: the link draws its bits and data noise exactly as before.

A frame is still a pure function of ``(seed, g)``.  The sources are independent with the statistics above, so
``E[H_a[s,t] conj(H_b[s',t'])] = (L L^H)[a][b] r_f(s-s') r_t(t-t')`` with ``L L^H = C_rx (x) C_tx`` up to the one float32 rounding of
``L``; the diagonal of ``L L^H`` is 1, so every frame ALONE has exactly the second-order statistics of an ungrouped frame (which is why
``lmmse.py`` needs no change).  ``simulate_frames_host`` evaluates this in float64 on the float32-rounded ``mix`` for any vector of frame
numbers, forming the sources it needs itself; ``aft_channel_sim_group_f32`` is the device's entry point.  With ``antennas = (1, 1)``
(the default) nothing above applies: frames are independent draws with their own conditions, bit for bit what they were.

Time continuity: slot sequences.  ``slots = K`` and ``slot_symbols = L`` (``None``: ``L = T``, back-to-back slots; ``L > T`` leaves a gap of
``L - T`` symbols between slots) make every ``K G`` consecutive frames K consecutive SLOTS of one fading process, ``K L <=
AFT_CHANSIM_MAX_SLOTS = 4096`` symbols.  Global frame ``g`` is in sequence ``seq = g // (K G)``, ``lead = seq K G``, slot
``k = (g - lead) // G``, member ``a = g % G``: slot-major, the antennas inside a slot, so a slot's G frames are exactly the group the links'
``branches=`` / ``streams=`` / ``precoding_subband=`` consume.  For frame ``g`` of a configuration with ``K > 1``:

* conditions: the three condition indices are picked from the SEQUENCE leader's key ``frame_keys(seed, lead)`` -- a whole sequence shares
  SNR, delay spread and Doppler (``frame_conditions``, ``SynthLoader``'s meta and ``make_pack`` follow);
* sources: ``z_j``, ``j = 0 .. a``, use the angle and phase streams of the key of frame ``lead + j`` -- the sequence's leader plus ``j``, the
  same rays in every slot;
* time: slot ``k`` evaluates the rays at the absolute symbol ``k L + t``.  So that float32 error does not grow in the sine's argument, a ray
  (turns per symbol ``rate``, phase ``phi`` in turns) first gets its slot's start phase ``phi_k = frac(fma(rate, float(k L), phi))``,
  ``frac(x) = x - floor(x)``, ``k L`` exact in float32; the phase in the slot is then ``fma(rate, t, phi_k)`` as for one slot.  With ``k = 0``
  ``phi_0 = phi`` exactly, ``phi`` lying in ``[0, 1)``.  The float64 twin does the same operations in float64;
* everything else is the grouped frame's: the mixing by ``L[a][j]``, the delay phasors and the sum over the taps, the pilot noise from frame
  ``g``'s OWN noise streams; the frame's key stays ``frame_keys(seed, g)``, so the links draw fresh bits and noise in every slot.

A frame is still a pure function of ``(seed, g)``, and ``E[H_k[s,t] conj(H_k'[s,t'])] = J0(2 pi f_D ((k - k') L + t - t') T_sym)``: the
slots of a sequence are one stretch of the process, which is what delayed feedback and retransmissions over a slow channel need.  A time
shift of rays with independent uniform phases is another draw of the same process, so every frame ALONE keeps exactly the second-order
statistics of an ungrouped frame (``lmmse.py`` and the estimators need no change).  ``simulate_frames_host`` evaluates this for any vector
of frame numbers; ``aft_channel_sim_seq_f32`` is the device's entry point, whose position arguments count SEQUENCES.  With ``slots = 1``
(the default) nothing of this paragraph applies, launch for launch.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Iterator, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _abi
from .synth import _DOP_GRID, _DS_GRID, _M64, _SNR_GRID, _splitmix64

# the streams of the counter-based hash (csrc/frame_device.h FrameStream): 0..4 the simulator's, 5..7 the link's, 8 the coded links'
# information bits, 9 the shifts of the default LDPC base matrix, keyed by its seed and used on the host only (linksim.py)
STREAM_CONDITION, STREAM_ANGLE, STREAM_PHASE, STREAM_NOISE_RADIUS, STREAM_NOISE_ANGLE = range(5)
STREAM_DATA_BITS, STREAM_DATA_NOISE_RADIUS, STREAM_DATA_NOISE_ANGLE = range(5, 8)
STREAM_CODE_BITS = 8
STREAM_LDPC_SHIFTS = 9
CHANNEL_TYPE = "SYNTH"


def _centred(n: int, k: int) -> Tuple[int, ...]:
    return tuple(i * (n // k) + (n // k) // 2 for i in range(k))


def _exponential_profile() -> np.ndarray:
    delay = 0.5 * np.arange(12)
    return np.stack([delay, 10.0 * np.log10(np.exp(-delay))], axis=1)


@dataclass(frozen=True)
class ChannelSimConfig:
    """What a frame is drawn from.  ``profile`` rows are (delay in multiples of the RMS delay spread, power in dB) -- the form of a 3GPP
    TDL table; the default is a 12-tap exponential profile, a user passes their own table.  ``pilot_scs`` / ``pilot_symbols`` default to
    evenly centred positions (subcarriers 5, 15, .., 115 and symbols 3, 10 on the default grid)."""
    ofdm: Tuple[int, int] = (120, 14)
    pilot: Tuple[int, int] = (12, 2)
    pilot_scs: Optional[Sequence[int]] = None
    pilot_symbols: Optional[Sequence[int]] = None
    subcarrier_spacing_hz: float = 15e3
    symbol_period_s: float = 1.0 / 14e3
    profile: Sequence = field(default_factory=_exponential_profile)
    rays: int = 8
    snr_db: Sequence[float] = tuple(float(v) for v in _SNR_GRID)
    delay_spread_ns: Sequence[float] = tuple(float(v) for v in _DS_GRID)
    doppler_hz: Sequence[float] = tuple(float(v) for v in _DOP_GRID)
    antennas: Tuple[int, int] = (1, 1)
    rx_correlation: Union[None, complex, Sequence] = None
    tx_correlation: Union[None, complex, Sequence] = None
    slots: int = 1
    slot_symbols: Optional[int] = None

    def __post_init__(self) -> None:
        S, T = (int(v) for v in self.ofdm)
        Ps, Pt = (int(v) for v in self.pilot)
        set_ = lambda k, v: object.__setattr__(self, k, v)  # noqa: E731
        set_("ofdm", (S, T))
        set_("pilot", (Ps, Pt))
        if S < 1 or T < 1:
            raise ValueError(f"ofdm grid {S} x {T}: both sizes must be at least 1")
        if not (1 <= Ps <= _abi.AFT_CHANSIM_MAX_PILOT_SCS and 1 <= Pt <= _abi.AFT_CHANSIM_MAX_PILOT_SYMBOLS and Ps <= S and Pt <= T):
            raise ValueError(f"pilot grid {Ps} x {Pt}: at most {_abi.AFT_CHANSIM_MAX_PILOT_SCS} x {_abi.AFT_CHANSIM_MAX_PILOT_SYMBOLS} "
                             f"and no larger than the ofdm grid {S} x {T}")
        for name, count, size in (("pilot_scs", Ps, S), ("pilot_symbols", Pt, T)):
            given = getattr(self, name)
            idx = _centred(size, count) if given is None else tuple(int(v) for v in given)
            if len(idx) != count or any(v < 0 or v >= size for v in idx) or any(b <= a for a, b in zip(idx, idx[1:])):
                raise ValueError(f"{name} = {list(idx)}: need {count} strictly increasing positions in [0, {size})")
            set_(name, idx)
        prof = np.array(self.profile, dtype=np.float64)
        if prof.ndim != 2 or prof.shape[1] != 2 or not 1 <= prof.shape[0] <= _abi.AFT_CHANSIM_MAX_TAPS or not np.isfinite(prof).all():
            raise ValueError(f"profile must be a finite [P, 2] table (normalised delay, power in dB) with 1 <= P <= "
                             f"{_abi.AFT_CHANSIM_MAX_TAPS}; got shape {prof.shape}")
        if (prof[:, 0] < 0).any():
            raise ValueError("profile delays must not be negative")
        prof.setflags(write=False)
        set_("profile", prof)
        if not 1 <= int(self.rays) <= _abi.AFT_CHANSIM_MAX_RAYS:
            raise ValueError(f"rays = {self.rays}: 1 to {_abi.AFT_CHANSIM_MAX_RAYS} sinusoids per tap")
        set_("rays", int(self.rays))
        for name in ("snr_db", "delay_spread_ns", "doppler_hz"):
            vals = tuple(float(v) for v in np.atleast_1d(np.asarray(getattr(self, name), dtype=np.float64)))
            if not 1 <= len(vals) <= _abi.AFT_CHANSIM_MAX_VALUES or not np.isfinite(vals).all():
                raise ValueError(f"{name} must list 1 to {_abi.AFT_CHANSIM_MAX_VALUES} finite values; got {len(vals)}")
            set_(name, vals)
        if min(self.delay_spread_ns) < 0 or min(self.doppler_hz) < 0:
            raise ValueError("delay_spread_ns and doppler_hz must not be negative")
        if not (self.subcarrier_spacing_hz > 0 and self.symbol_period_s > 0):
            raise ValueError("subcarrier_spacing_hz and symbol_period_s must be positive")
        try:
            R, N = (int(v) for v in self.antennas)
        except (TypeError, ValueError):
            raise ValueError(f"antennas = {self.antennas!r}: need (receive antennas, transmit streams)") from None
        if R < 1 or N < 1 or R * N > _abi.AFT_CHANSIM_MAX_GROUP:
            raise ValueError(f"antennas = ({R}, {N}): both at least 1 and at most {_abi.AFT_CHANSIM_MAX_GROUP} frames in a group")
        set_("antennas", (R, N))
        set_("rx_correlation", _correlation("rx_correlation", self.rx_correlation, R))
        set_("tx_correlation", _correlation("tx_correlation", self.tx_correlation, N))
        K, L = self.slots, T if self.slot_symbols is None else self.slot_symbols
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (K, L)) or K < 1:
            raise ValueError(f"slots = {self.slots!r}, slot_symbols = {self.slot_symbols!r}: slots an integer of at least 1, slot_symbols "
                             f"an integer or None")
        if L < T:
            raise ValueError(f"slot_symbols = {L}: a slot spans at least the {T} symbols of the grid")
        if K > 1 and K * L > _abi.AFT_CHANSIM_MAX_SLOTS:
            raise ValueError(f"slots * slot_symbols = {K} * {L}: a sequence spans at most {_abi.AFT_CHANSIM_MAX_SLOTS} symbols")
        set_("slots", int(K))
        set_("slot_symbols", int(L))

    @property
    def group(self) -> int:
        """G = R N: the frames of one receiver."""
        return self.antennas[0] * self.antennas[1]

    def sequence(self) -> int:
        """K G: the frames of one slot sequence (the group's G with ``slots = 1``)."""
        return self.slots * self.group

    def mix(self) -> np.ndarray:
        """complex64 ``[G, G]``: ``kron(chol(C_rx), chol(C_tx))``, formed in float64 and rounded once; lower triangular."""
        chol = lambda c, n: np.eye(n, dtype=np.complex128) if c is None else np.linalg.cholesky(_matrix(c, n))  # noqa: E731
        return np.kron(chol(self.rx_correlation, self.antennas[0]), chol(self.tx_correlation, self.antennas[1])).astype(np.complex64)

    def tables(self) -> Dict[str, np.ndarray]:
        """The numbers the definition works with, rounded to float32 exactly as ``aft_chansim`` carries them."""
        power = 10.0 ** (self.profile[:, 1] / 10.0)
        f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32)  # noqa: E731
        ds, dop = f32(self.delay_spread_ns), f32(self.doppler_hz)
        return {
            "tap_delay": f32(self.profile[:, 0]),
            "tap_amp": f32(np.sqrt(power / power.sum() / self.rays)),
            "snr_db": f32(self.snr_db),
            "noise_sigma": f32(10.0 ** (-np.asarray(self.snr_db) / 20.0)),
            "delay_spread_ns": ds,
            "doppler_hz": dop,
            # the launcher forms these two the same way: double products, one rounding
            "delay_turns": (np.float64(self.subcarrier_spacing_hz) * ds.astype(np.float64) * 1e-9).astype(np.float32),
            "doppler_turns": (dop.astype(np.float64) * np.float64(self.symbol_period_s)).astype(np.float32),
            "mix": self.mix(),
        }

    def fill_grid(self, struct):
        """The OFDM grid, the pilot grid and the pilot positions into a struct that carries them (``aft_chansim``, ``aft_link``)."""
        struct.num_scs, struct.num_symbols = self.ofdm
        struct.pilot_scs, struct.pilot_symbols = self.pilot
        struct.pilot_sc_index[:len(self.pilot_scs)] = self.pilot_scs
        struct.pilot_symbol_index[:len(self.pilot_symbols)] = self.pilot_symbols
        return struct

    def to_struct(self) -> "_abi.AftChanSim":
        t = self.tables()
        sim = self.fill_grid(_abi.AftChanSim())
        sim.taps, sim.rays = len(t["tap_delay"]), self.rays
        sim.n_snr, sim.n_ds, sim.n_dop = len(self.snr_db), len(self.delay_spread_ns), len(self.doppler_hz)
        sim.subcarrier_spacing_hz, sim.symbol_period_s = float(self.subcarrier_spacing_hz), float(self.symbol_period_s)
        for name in ("tap_delay", "tap_amp", "snr_db", "noise_sigma", "delay_spread_ns", "doppler_hz"):
            arr = getattr(sim, name)
            for i, v in enumerate(t[name]):
                arr[i] = float(v)
        return sim


def _matrix(c, n: int) -> np.ndarray:
    """The [n, n] correlation matrix of a validated correlation: the exponential model of a scalar, or the matrix itself."""
    if isinstance(c, np.ndarray):
        return c
    i = np.arange(n)
    d = i[:, None] - i[None, :]
    return np.where(d >= 0, complex(c) ** np.maximum(d, 0), np.conj(complex(c)) ** np.maximum(-d, 0))


def _correlation(name: str, given, n: int):
    """A correlation as the config keeps it: None, a complex scalar, or a read-only complex128 [n, n] matrix; ValueError otherwise."""
    if given is None:
        return None
    try:
        c = np.asarray(given, dtype=np.complex128)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: not a number or a matrix of numbers") from None
    if not np.isfinite(c).all():
        raise ValueError(f"{name} has a non-finite entry")
    if n == 1:
        if (c.ndim == 0 and c == 0) or (c.shape == (1, 1) and abs(c[0, 0] - 1) <= 1e-12):
            return None                                          # the trivial correlation of one antenna
        raise ValueError(f"{name} given for a dimension of size 1")
    if c.ndim == 0:
        if not abs(c) < 1:
            raise ValueError(f"{name} = {complex(c)}: the exponential model needs |rho| < 1")
        return complex(c)
    if c.shape != (n, n):
        raise ValueError(f"{name} has shape {c.shape}: need a scalar or a [{n}, {n}] matrix")
    if np.abs(c - c.conj().T).max() > 1e-12 or np.abs(np.diag(c) - 1).max() > 1e-12:
        raise ValueError(f"{name} must be Hermitian with a unit diagonal (to 1e-12)")
    try:
        np.linalg.cholesky(c)
    except np.linalg.LinAlgError:
        raise ValueError(f"{name} is not positive definite") from None
    c = c.copy()
    c.setflags(write=False)
    return c


# ---- the hash: written once, mirrored by csrc/frame_device.h ----------------------------------------------------------------

def frame_keys(seed: int, frame_ids) -> np.ndarray:
    """``sm(sm(seed) ^ g)`` per frame, uint64."""
    g = np.asarray(frame_ids, dtype=np.int64)
    if g.ndim != 1 or (g < 0).any():
        raise ValueError("frame_ids must be a vector of non-negative frame numbers")
    sk = _splitmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]
    return _splitmix64(sk ^ g.astype(np.uint64))


def words(keys: np.ndarray, stream: int, index) -> np.ndarray:
    """64-bit words of ``stream`` at ``index`` (broadcast against ``keys``)."""
    tag = (np.uint64(stream) << np.uint64(32)) | np.asarray(index, dtype=np.uint64)
    return _splitmix64((keys ^ tag) & _M64)


def _pick(keys: np.ndarray, which: int, n: int) -> np.ndarray:
    return (((words(keys, STREAM_CONDITION, which) >> np.uint64(40)) * np.uint64(n)) >> np.uint64(24)).astype(np.int64)


def frame_conditions(cfg: ChannelSimConfig, seed: int, frame_ids) -> np.ndarray:
    """float32 ``[n, 3]``: the (snr_db, delay_spread_ns, doppler_hz) of each frame -- integer arithmetic on the hash, so host and
    device agree exactly.  With a grouped configuration they are the LEADER's: one pick per group, and one per sequence with ``slots > 1``."""
    return _conditions(cfg.tables(), frame_keys(seed, _leaders(cfg, frame_ids)))[0]


def _leaders(cfg: ChannelSimConfig, frame_ids) -> np.ndarray:
    """The frame whose key picks each frame's conditions: the frame itself, or the first of its group (of its sequence)."""
    g = np.asarray(frame_ids, dtype=np.int64)
    return g if cfg.sequence() == 1 else g - g % cfg.sequence()


def _conditions(t: Dict[str, np.ndarray], keys: np.ndarray):
    """(meta float32 [n, 3], the three index vectors) from the keys that pick the conditions: the LEADERS' with a grouped configuration."""
    idx = [_pick(keys, k, len(t[name])) for k, name in enumerate(("snr_db", "delay_spread_ns", "doppler_hz"))]
    meta = np.stack([t["snr_db"][idx[0]], t["delay_spread_ns"][idx[1]], t["doppler_hz"][idx[2]]], axis=1).astype(np.float32)
    return meta, idx


def simulate_frames_host(cfg: ChannelSimConfig, seed: int, frame_ids, return_noise: bool = False):
    """The definition in float64: ``(ideal complex128 [n,S,T], pilots complex128 [n,Ps,Pt], meta float32 [n,3])`` for the given global
    frame numbers (and the noise that was added, complex128 ``[n,Ps,Pt]``, with ``return_noise``).  Needs no library."""
    t = cfg.tables()
    keys = frame_keys(seed, frame_ids)
    n = len(keys)
    S, T = cfg.ofdm
    Ps, Pt = cfg.pilot
    P, M = len(t["tap_delay"]), cfg.rays
    G, K = cfg.group, cfg.slots
    meta, (i_snr, i_ds, i_dop) = _conditions(t, keys if G * K == 1 else frame_keys(seed, _leaders(cfg, frame_ids)))

    def tap_gains(kk, i_dop, first=None):                        # [len(kk),P,T]; first: the slots' first absolute symbols, k L
        kk = kk[:, None, None]
        ray = (16 * np.arange(P)[:, None] + np.arange(M)[None, :])[None]                                   # [1,P,M]
        u = (words(kk, STREAM_ANGLE, ray) >> np.uint64(44)).astype(np.float64) * 2.0 ** -20
        phase = (words(kk, STREAM_PHASE, ray) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24            # turns
        rate = t["doppler_turns"].astype(np.float64)[i_dop][:, None, None] * np.cos(2.0 * np.pi * (np.arange(M)[None, None, :] + u) / M)
        if first is not None:                                    # the slot's start phase, reduced: phi_k = frac(rate k L + phi)
            phase = rate * first.astype(np.float64)[:, None, None] + phase
            phase = phase - np.floor(phase)
        turns = rate[..., None] * np.arange(T)[None, None, None, :] + phase[..., None]                     # [n,P,M,T]
        return t["tap_amp"].astype(np.float64)[None, :, None] * np.exp(2j * np.pi * (turns - np.floor(turns))).sum(axis=2)

    if G * K == 1:
        gain = tap_gains(keys, i_dop)
    else:                                                        # the sources of every group that occurs, once; then row a of `mix`
        g = np.asarray(frame_ids, dtype=np.int64)
        unit, where = np.unique(g // G, return_inverse=True)    # a group: slot unit % K of the sequence unit // K
        lead = unit // K * (K * G)                               # the sources' keys are the sequence leader's plus j, whatever the slot
        dop_of = np.empty(len(unit), dtype=np.int64)
        dop_of[where] = i_dop
        first = np.repeat(unit % K * cfg.slot_symbols, G) if K > 1 else None
        z = tap_gains(frame_keys(seed, (lead[:, None] + np.arange(G)[None, :]).ravel()), np.repeat(dop_of, G), first)
        z = z.reshape(len(unit), G, P, T)
        gain = np.einsum("nj,njpt->npt", t["mix"].astype(np.complex128)[g % G], z[where]) if G > 1 else z[where, 0]
    per_sc = t["delay_turns"].astype(np.float64)[i_ds][:, None] * t["tap_delay"].astype(np.float64)[None, :]             # [n,P]
    x = per_sc[:, :, None] * np.arange(S)[None, None, :]                                                   # [n,P,S]
    phasor = np.exp(-2j * np.pi * (x - np.floor(x)))
    ideal = np.einsum("nps,npt->nst", phasor, gain)
    q = np.arange(Ps * Pt)[None, :]
    k1 = (words(keys[:, None], STREAM_NOISE_RADIUS, q) >> np.uint64(41)).astype(np.float64)
    k2 = (words(keys[:, None], STREAM_NOISE_ANGLE, q) >> np.uint64(41)).astype(np.float64)
    u1, u2 = (k1 + 0.5) * 2.0 ** -23, (k2 + 0.5) * 2.0 ** -23
    sigma = t["noise_sigma"].astype(np.float64)[i_snr][:, None]
    noise = (sigma * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)).reshape(n, Ps, Pt)
    pilots = ideal[:, np.asarray(cfg.pilot_scs)[:, None], np.asarray(cfg.pilot_symbols)[None, :]] + noise
    return (ideal, pilots, meta, noise) if return_noise else (ideal, pilots, meta)


def _pinned(cfg: ChannelSimConfig, snr_db=None, delay_spread_ns=None, doppler_hz=None) -> ChannelSimConfig:
    import dataclasses
    over = {k: (float(v),) for k, v in (("snr_db", snr_db), ("delay_spread_ns", delay_spread_ns), ("doppler_hz", doppler_hz))
            if v is not None}
    return dataclasses.replace(cfg, **over) if over else cfg


def make_pack(cfg: ChannelSimConfig, n: int, seed: int, snr_db=None, delay_spread_ns=None, doppler_hz=None) -> Dict[str, np.ndarray]:
    """Frames ``[0, n)`` of ``seed`` as a pack in ``ingest.pack_mat_folder``'s format (``h_ideal``, ``h_ls_sparse``, ``h_ls_full``,
    ``meta [n,5]`` = (frame number, snr, ds, dop, 0), ``channel_type`` "SYNTH"), any condition pinned to one value: fixed validation
    and test sets per condition for ``PackedLoader`` / ``ResidentLoader`` / ``get_test_stats`` / the LS-baseline kernel.
    ``h_ls_full`` is the pilots' LS estimate interpolated linearly over the grid (held constant outside the pilots' span), the baseline
    an estimator has to beat."""
    if n < 1:
        raise ValueError(f"make_pack needs n >= 1 (got {n})")
    if n % cfg.sequence():
        raise ValueError(f"make_pack needs whole {'groups' if cfg.slots == 1 else 'sequences'}: n = {n} is not a multiple of the "
                         f"{cfg.sequence()} frames of {_unit_text(cfg)}")
    cfg = _pinned(cfg, snr_db, delay_spread_ns, doppler_hz)
    ideal, pilots, cond = simulate_frames_host(cfg, seed, np.arange(n))
    ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
    if (pilots == 0).any():                                      # a pilot of exactly zero would vanish from the sparse grid
        raise ValueError("a simulated pilot is exactly zero: choose another seed")
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    sparse = np.zeros_like(ideal)
    sparse[:, sc[:, None], sym[None, :]] = pilots
    meta = np.zeros((n, 5), np.float32)
    meta[:, 0] = np.arange(n)
    meta[:, 1:4] = cond
    return {"h_ideal": ideal, "h_ls_sparse": sparse, "h_ls_full": ls_interpolate(cfg, pilots), "meta": meta,
            "channel_type": np.asarray([CHANNEL_TYPE] * n)}


def _unit_text(cfg: ChannelSimConfig) -> str:
    """What the frames of one unit -- a group, or a sequence of slots of groups -- are the frames of, for an error message."""
    return f"antennas = {cfg.antennas}" if cfg.slots == 1 else f"slots = {cfg.slots} x antennas = {cfg.antennas}"


def ls_interpolate(cfg: ChannelSimConfig, pilots: np.ndarray) -> np.ndarray:
    """Pilots ``[n,Ps,Pt]`` -> complex64 ``[n,S,T]``: linear interpolation along the subcarriers, then along the symbols."""
    S, T = cfg.ofdm
    sc, sym = np.asarray(cfg.pilot_scs, dtype=np.float64), np.asarray(cfg.pilot_symbols, dtype=np.float64)

    def weights(at: np.ndarray, size: int) -> np.ndarray:       # [size, len(at)] interpolation matrix, clamped at the ends
        w = np.zeros((size, len(at)))
        for i in range(size):
            if len(at) == 1 or i <= at[0]:
                w[i, 0] = 1.0
            elif i >= at[-1]:
                w[i, -1] = 1.0
            else:
                k = int(np.searchsorted(at, i, side="right")) - 1
                f = (i - at[k]) / (at[k + 1] - at[k])
                w[i, k], w[i, k + 1] = 1.0 - f, f
        return w

    return np.einsum("si,nij,tj->nst", weights(sc, S), pilots.astype(np.complex128), weights(sym, T)).astype(np.complex64)


class SynthLoader:
    """Training batches from the simulator, in the format ``ingest.ResidentLoader`` yields: ``(pilots complex64 [b,Ps,Pt], h_ideal
    complex64 [b,S,T]`` on ``device``, ``(file_no, snr, ds, dop, n: float32 [b,1] host tensors, [tuple of b "SYNTH" strings]))``;
    ``file_no`` is the frame's global number, ``n`` is 0.  ``file_no`` is informational (the model reads snr, ds and dop only) and, being
    float32 like the reference's, exact only below 2^24: 256 epochs of 65 536 fresh frames.  ``epoch_frames`` gives the exact numbers.

    An epoch is ``frames_per_epoch`` positions.  Rank ``r`` of ``world_size`` takes positions ``r, r + W, ..`` and wraps round the
    epoch where ``DistributedSampler`` pads (``drop_last``: the epoch is cut to a multiple of W instead, and a ragged last batch is
    dropped as well); position q of epoch e is global frame ``e * frames_per_epoch + q`` with ``fresh_each_epoch`` (data never runs
    out) and frame ``q`` without (every epoch replays ``[0, n)``).  Frames are independent draws, so there is nothing to shuffle.
    Every ``iter(loader)`` runs epoch ``loader.epoch`` and adds one to it; ``set_epoch`` rewinds, as ``ResidentLoader``'s does.

    On a HIP device a batch is one launch of ``aft_channel_sim_f32`` on the consumer's current stream plus the host's own evaluation
    of the same hash for the meta tensors: no device read, no ``.item()``, no side stream, no copy in either direction.  On
    ``device="cpu"`` the float64 definition is evaluated and rounded to complex64.

    With a grouped configuration (``cfg.antennas``, G frames per group) the unit of all of the above is the GROUP: ``batch_size`` and
    ``frames_per_epoch`` must be multiples of G, the ranks share out, wrap and drop whole groups, ``epoch_frames`` returns whole groups in
    order, and a batch is one launch of ``aft_channel_sim_group_f32``.  With G = 1 nothing changes.  With slot sequences (``cfg.slots``
    = K > 1) the unit is the SEQUENCE of ``K G`` frames in the same way, and a batch is one launch of ``aft_channel_sim_seq_f32``."""

    def __init__(self, cfg: ChannelSimConfig, batch_size: int, frames_per_epoch: int, device: Union[str, torch.device] = "cpu",
                 seed: int = 0, rank: int = 0, world_size: int = 1, drop_last: bool = False, fresh_each_epoch: bool = True) -> None:
        if batch_size < 1 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f"bad batch_size / rank / world_size: {batch_size} / {rank} / {world_size}")
        if frames_per_epoch < 1:
            raise ValueError(f"frames_per_epoch must be at least 1 (got {frames_per_epoch})")
        self.cfg, self.batch_size, self.n = cfg, int(batch_size), int(frames_per_epoch)
        self._G = cfg.sequence()                                 # the unit: a group, or a sequence of slots of groups
        if self.batch_size % self._G or self.n % self._G:
            raise ValueError(f"batch_size = {batch_size} and frames_per_epoch = {frames_per_epoch} must be multiples of the {self._G} "
                             f"frames of {_unit_text(cfg)}")
        self.device = torch.device(device)
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self.drop_last, self.fresh_each_epoch = bool(drop_last), bool(fresh_each_epoch)
        self.epoch = 0
        self._tables = cfg.tables()
        self._plan = None
        if self.device.type == "cuda":
            from .hip_ops import ChannelSimPlan
            self._plan = ChannelSimPlan(cfg, self.device)
            self.device = self._plan.device

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _samples(self) -> int:                                  # this rank's groups of an epoch (frames, with G = 1)
        units = self.n // self._G
        return units // self.world_size if self.drop_last else -(-units // self.world_size)

    def __len__(self) -> int:
        m, per_batch = self._samples(), self.batch_size // self._G
        return m // per_batch if self.drop_last else -(-m // per_batch)

    def epoch_frames(self, epoch: int) -> np.ndarray:
        """The global frame numbers this rank visits in ``epoch``, in order (int64): whole groups with a grouped configuration."""
        G, units = self._G, self.n // self._G
        count = len(self) * (self.batch_size // G) if self.drop_last else self._samples()
        base = epoch * units if self.fresh_each_epoch else 0
        group = base + (self.rank + self.world_size * np.arange(count, dtype=np.int64)) % units
        return group if G == 1 else (group[:, None] * G + np.arange(G, dtype=np.int64)[None, :]).ravel()

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor, tuple]]:
        epoch, self.epoch = self.epoch, self.epoch + 1
        return self._batches(epoch)

    def _meta(self, frames: np.ndarray) -> tuple:
        cond = _conditions(self._tables, frame_keys(self.seed, _leaders(self.cfg, frames)))[0]
        m = torch.from_numpy(np.concatenate([frames.astype(np.float32)[:, None], cond, np.zeros((len(frames), 1), np.float32)], axis=1))
        return (m[:, 0:1], m[:, 1:2], m[:, 2:3], m[:, 3:4], m[:, 4:5], [tuple(CHANNEL_TYPE for _ in frames)])

    def _batches(self, epoch: int):
        frames = self.epoch_frames(epoch)
        G, units = self._G, self.n // self._G                    # the launch counts groups: positions, base and modulo in groups
        base = epoch * units if self.fresh_each_epoch else 0
        for lo in range(0, len(frames), self.batch_size):
            part = frames[lo:lo + self.batch_size]
            if self._plan is None:
                ideal, pilots, _ = simulate_frames_host(self.cfg, self.seed, part)
                yield torch.from_numpy(pilots.astype(np.complex64)), torch.from_numpy(ideal.astype(np.complex64)), self._meta(part)
                continue
            args = (self.seed, base, self.rank + self.world_size * (lo // G), self.world_size, units, len(part))
            if torch.cuda.current_device() != self.device.index:    # the launch belongs to the loader's device, whichever is current
                with torch.cuda.device(self.device):
                    ideal, pilots, _ = self._plan(*args)
            else:
                ideal, pilots, _ = self._plan(*args)
            yield pilots, ideal, self._meta(part)
