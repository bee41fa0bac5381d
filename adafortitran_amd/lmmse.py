"""The LMMSE (Wiener) estimator of the simulator's channel: the baseline a trained estimator is compared with.

``chansim`` defines the channel's second-order statistics exactly -- ``E|H|^2 = 1``, time correlation ``J0(2 pi f_D k T_sym)``,
frequency correlation ``sum_p pw_p exp(-j 2 pi d df d_p DS)`` -- so the best LINEAR estimator of the grid from the noisy pilots can be
written down, per (SNR, delay spread, Doppler).  This module DEFINES it, in float64 on the float32-rounded numbers of
``ChannelSimConfig.tables()`` (the numbers the device sees, so the device's error is arithmetic only):

* ``LmmseTables`` holds the tables; ``lmmse_estimate_host`` evaluates the definition (the CPU path and the yardstick);
* ``lmmse_predicted_mse`` is the closed-form MSE, matched or mismatched;
* ``aft_lmmse_f32`` (csrc/k_lmmse.hip, through ``hip_ops.LmmsePlan``) evaluates it in float32 on the device, one launch per batch;
* ``LmmseEstimator`` is the ``nn.Module`` the evaluation sweep (``evaluation.get_test_stats``) measures like any other estimator.

The definition.  ``sc_i`` / ``sym_j`` the pilot positions, ``pw_p = tap_amp_p^2 rays`` the tap powers, ``sigma2 = 10^(-snr_db / 10)``::

    r_f(d; i_ds)  = sum_p pw_p exp(-j 2 pi d delay_turns[i_ds] tap_delay_p)          r_t(k; i_dop) = J0(2 pi doppler_turns[i_dop] k)
    R_f = r_f(sc_i - sc_i') = U_f diag(lf) U_f^H      F' = r_f(s - sc_i) U_f   [S, Ps]       (per delay spread)
    R_t = r_t(sym_j - sym_j') = U_t diag(lt) U_t^T    T' = r_t(t - sym_j) U_t  [T, Pt]       (per Doppler)
    est = F' [ D o (U_f^H P U_t) ] T'^T,      D[k][l] = 1 / (lf[k] lt[l] + sigma2),      P the frame's [Ps, Pt] pilots

which is ``R_hp (R_pp + sigma2 I)^-1 p`` with ``R_pp = R_f (x) R_t`` written in the Kronecker eigenbasis: no inverse is formed (in
float32 the inverse loses 5e-4 of |est|max where cond(R_pp + sigma2 I) is 2e4; the eigenbasis form stays at float32's own rounding),
and the tables are per delay spread and per Doppler, never per condition triple.  Eigenvalues are clamped at 0 from below.

Which design point a frame uses: per condition the index of the NEAREST table value (``|v - value[i]|`` in float64, ties to the lower
index, NaN to index 0) -- a total function, no error path; ``assume=dict(snr_db=.., delay_spread_ns=.., doppler_hz=..)`` pins any of the
three for every frame, whatever its meta says (the mismatched, or robust, receiver); a pinned value is chosen by nearest value too.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _abi
from .chansim import ChannelSimConfig

CONDITIONS = ("snr_db", "delay_spread_ns", "doppler_hz")


def j0(x, n: Optional[int] = None) -> np.ndarray:
    """Bessel J0 in float64 without a dependency: ``mean_n cos(x cos(theta_n))``, ``theta_n = 2 pi (n + 1/2) / N`` -- the midpoint rule
    on a periodic analytic integrand, which converges geometrically once ``N`` exceeds ``|x|``; ``N >= 2 |x|max + 64`` (512 at least)
    is exact to ~1e-15."""
    x = np.asarray(x, dtype=np.float64)
    need = int(np.ceil(2.0 * float(np.abs(x).max(initial=0.0)) + 64.0))
    n = max(512, need) if n is None else int(n)
    if n < need:
        raise ValueError(f"j0: N = {n} points is too few for |x| up to {float(np.abs(x).max()):.3g} (need {need})")
    c = np.cos(2.0 * np.pi * (np.arange(n) + 0.5) / n)
    flat = x.reshape(-1)
    out = np.empty_like(flat)
    step = max(1, (1 << 22) // n)                                # 32 MB of cosines at a time
    for lo in range(0, flat.size, step):
        out[lo:lo + step] = np.cos(flat[lo:lo + step, None] * c[None, :]).mean(axis=1)
    return out.reshape(x.shape)


def nearest_index(values, v) -> np.ndarray:
    """Index of the entry of ``values`` nearest to each ``v``: float64 distances, ties to the lower index, NaN to 0 (int64, v's shape)."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    v = np.asarray(v, dtype=np.float64)
    best = np.zeros(v.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        bd = np.abs(v - values[0])
        for i in range(1, len(values)):
            d = np.abs(v - values[i])
            closer = d < bd                                       # False for a NaN: the scan of k_lmmse.hip, line for line
            best = np.where(closer, i, best)
            bd = np.where(closer, d, bd)
    return best


def _check_assume(assume) -> Dict[str, float]:
    if assume is None:
        return {}
    if not isinstance(assume, dict) or any(k not in CONDITIONS for k in assume):
        raise ValueError(f"assume must be a dict with keys from {CONDITIONS}; got {assume!r}")
    out = {}
    for k, val in assume.items():
        if val is None:
            continue
        val = np.asarray(val, dtype=np.float64)
        if val.ndim != 0 or not np.isfinite(val):
            raise ValueError(f"assume[{k!r}] must be one finite number; got {assume[k]!r}")
        out[k] = float(val)
    return out


class LmmseTables:
    """The estimator's tables for one ``ChannelSimConfig``: float64 (``sigma2 [n_snr]``; per delay spread ``lam_f [Ps]``, ``u_f
    [Ps, Ps]``, ``f [S, Ps]`` = F'; per Doppler ``lam_t [Pt]``, ``u_t [Pt, Pt]``, ``t [T, Pt]`` = T') and ``image()``, the float32
    array ``aft_lmmse_f32`` reads (include/adafortitran_amd.h documents its layout)."""

    def __init__(self, cfg: ChannelSimConfig) -> None:
        if not isinstance(cfg, ChannelSimConfig):
            raise ValueError(f"LmmseTables needs a chansim.ChannelSimConfig (got {type(cfg).__name__})")
        self.cfg = cfg
        t = cfg.tables()
        S, T = cfg.ofdm
        self.values = {k: t[k].astype(np.float64) for k in CONDITIONS}
        self.sigma2 = 10.0 ** (-self.values["snr_db"] / 10.0)
        self.pw = t["tap_amp"].astype(np.float64) ** 2 * cfg.rays
        self.tap_delay = t["tap_delay"].astype(np.float64)
        self.delay_turns, self.doppler_turns = t["delay_turns"].astype(np.float64), t["doppler_turns"].astype(np.float64)
        self.sc, self.sym = np.asarray(cfg.pilot_scs, dtype=np.int64), np.asarray(cfg.pilot_symbols, dtype=np.int64)
        self.lam_f, self.u_f, self.f = [], [], []
        for i in range(len(self.delay_turns)):
            lam, u = np.linalg.eigh(self.r_f(self.sc[:, None] - self.sc[None, :], i))
            self.lam_f.append(np.maximum(lam, 0.0))
            self.u_f.append(u)
            self.f.append(self.r_f(np.arange(S)[:, None] - self.sc[None, :], i) @ u)
        self.lam_t, self.u_t, self.t = [], [], []
        for i in range(len(self.doppler_turns)):
            lam, u = np.linalg.eigh(self.r_t(self.sym[:, None] - self.sym[None, :], i))
            self.lam_t.append(np.maximum(lam, 0.0))
            self.u_t.append(u)
            self.t.append(self.r_t(np.arange(T)[:, None] - self.sym[None, :], i) @ u)

    def r_f(self, d, i_ds: int) -> np.ndarray:
        """Frequency correlation at subcarrier lag ``d`` (complex128, d's shape)."""
        d = np.asarray(d, dtype=np.float64)
        return (self.pw * np.exp(-2j * np.pi * d[..., None] * (self.delay_turns[i_ds] * self.tap_delay))).sum(axis=-1)

    def r_t(self, k, i_dop: int) -> np.ndarray:
        """Time correlation at symbol lag ``k`` (float64, k's shape)."""
        return j0(2.0 * np.pi * self.doppler_turns[i_dop] * np.asarray(k, dtype=np.float64))

    def indices(self, conditions, assume=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The (i_snr, i_ds, i_dop) design point of each row of ``conditions [n, 3]`` = (snr_db, delay_spread_ns, doppler_hz)."""
        fixed = self.fixed(assume)
        cond = np.asarray(conditions, dtype=np.float64)
        if cond.ndim != 2 or cond.shape[1] != 3:
            raise ValueError(f"conditions must be [n, 3] = (snr_db, delay_spread_ns, doppler_hz); got shape {cond.shape}")
        return tuple(np.full(len(cond), fixed[k], dtype=np.int64) if fixed[k] >= 0 else nearest_index(self.values[name], cond[:, k])
                     for k, name in enumerate(CONDITIONS))

    def fixed(self, assume=None) -> Tuple[int, int, int]:
        """The three pinned indices of ``assume`` (-1: from the frame)."""
        a = _check_assume(assume)
        return tuple(int(nearest_index(self.values[name], a[name])) if name in a else -1 for name in CONDITIONS)

    def gain(self, i_snr: int, i_ds: int, i_dop: int) -> np.ndarray:
        """D [Ps, Pt] of a design point."""
        return 1.0 / (self.lam_f[i_ds][:, None] * self.lam_t[i_dop][None, :] + self.sigma2[i_snr])

    def image(self) -> np.ndarray:
        """The float32 table image of ``aft_lmmse_f32``."""
        Ps = self.cfg.pilot[0]
        pairs = lambda z: np.stack([z.real, z.imag], axis=-1).reshape(-1)  # noqa: E731
        parts = []
        for lam, u, f in zip(self.lam_f, self.u_f, self.f):
            parts += [pairs(u.conj().T), pairs(f.T), lam, np.zeros(Ps & 1)]
        for lam, u, t in zip(self.lam_t, self.u_t, self.t):
            parts += [u.reshape(-1), t.T.reshape(-1), lam]
        return np.concatenate(parts).astype(np.float32)

    def to_struct(self, assume=None) -> "_abi.AftLmmse":
        p = _abi.AftLmmse()
        p.num_scs, p.num_symbols = self.cfg.ofdm
        p.pilot_scs, p.pilot_symbols = self.cfg.pilot
        p.n_snr, p.n_ds, p.n_dop = (len(self.values[k]) for k in CONDITIONS)
        p.fixed_snr, p.fixed_ds, p.fixed_dop = self.fixed(assume)
        for name in CONDITIONS:
            for i, v in enumerate(self.values[name]):
                getattr(p, name)[i] = float(v)
        for i, v in enumerate(self.sigma2.astype(np.float32)):
            p.noise_var[i] = float(v)
        return p


def _tables(cfg: Union[ChannelSimConfig, LmmseTables]) -> LmmseTables:
    return cfg if isinstance(cfg, LmmseTables) else LmmseTables(cfg)


def lmmse_estimate_host(cfg: Union[ChannelSimConfig, LmmseTables], pilots, conditions, assume=None) -> np.ndarray:
    """The definition in float64: pilots ``[n, Ps, Pt]`` and conditions ``[n, 3]`` = (snr_db, delay_spread_ns, doppler_hz) ->
    complex128 ``[n, S, T]``.  ``cfg`` may be an ``LmmseTables`` (built once, used for many calls).  Needs no library."""
    tb = _tables(cfg)
    pilots = np.asarray(pilots).astype(np.complex128)
    if pilots.ndim != 3 or pilots.shape[1:] != tuple(tb.cfg.pilot):
        raise ValueError(f"Expected pilot shape (n, {tb.cfg.pilot[0]}, {tb.cfg.pilot[1]}), got {pilots.shape}")
    if conditions is None:
        if min(tb.fixed(assume)) < 0:
            raise ValueError("conditions are required unless assume pins all three")
        conditions = np.zeros((len(pilots), 3))
    i_snr, i_ds, i_dop = tb.indices(conditions, assume)
    if len(i_snr) != len(pilots):
        raise ValueError(f"{len(pilots)} frames but {len(i_snr)} rows of conditions")
    out = np.empty((len(pilots), *tb.cfg.ofdm), dtype=np.complex128)
    key = i_snr * 1024 + i_ds * 32 + i_dop
    for k in np.unique(key):
        sel = np.nonzero(key == k)[0]
        a, d, e = int(i_snr[sel[0]]), int(i_ds[sel[0]]), int(i_dop[sel[0]])
        y = np.einsum("ik,nij,jl->nkl", tb.u_f[d].conj(), pilots[sel], tb.u_t[e]) * tb.gain(a, d, e)[None]
        out[sel] = np.einsum("sk,nkl,tl->nst", tb.f[d], y, tb.t[e])
    return out


def lmmse_predicted_mse(cfg: Union[ChannelSimConfig, LmmseTables], snr_db: float, delay_spread_ns: float, doppler_hz: float,
                        assume=None) -> float:
    """The closed-form MSE per grid element of the estimator on frames drawn at the given condition (its nearest table values).
    Matched: ``1 - (1 / ST) sum_{s,t} sum_{k,l} |F'_sk|^2 T'_tl^2 D_kl``.  With ``assume`` the estimator ``W`` is that of the pinned
    design while the statistics are the true ones: ``1 - 2 Re diag(W R_ph) + diag(W (R_pp + sigma2 I) W^H)``, averaged over the grid
    (full matrices: host only)."""
    tb = _tables(cfg)
    true = tuple(int(v[0]) for v in tb.indices([[snr_db, delay_spread_ns, doppler_hz]]))
    used = tuple(int(v[0]) for v in tb.indices([[snr_db, delay_spread_ns, doppler_hz]], assume))
    S, T = tb.cfg.ofdm
    if used == true:
        a, d, e = true
        return float(1.0 - np.einsum("sk,tl,kl->", np.abs(tb.f[d]) ** 2, tb.t[e] ** 2, tb.gain(a, d, e)) / (S * T))
    a, d, e = used
    w = (np.kron(tb.f[d], tb.t[e]) * tb.gain(a, d, e).reshape(-1)[None, :]) @ np.kron(tb.u_f[d], tb.u_t[e]).conj().T      # [ST, PsPt]
    a, d, e = true
    s, t = np.arange(S), np.arange(T)
    r_ph = np.kron(tb.r_f(tb.sc[:, None] - s[None, :], d), tb.r_t(tb.sym[:, None] - t[None, :], e))                        # [PsPt, ST]
    r_pp = np.kron(tb.r_f(tb.sc[:, None] - tb.sc[None, :], d), tb.r_t(tb.sym[:, None] - tb.sym[None, :], e))
    r_pp = r_pp + tb.sigma2[a] * np.eye(len(r_pp))
    per = 1.0 - 2.0 * np.real((w * r_ph.T).sum(axis=1)) + np.real(((w @ r_pp) * w.conj()).sum(axis=1))
    return float(per.mean())


class LmmseEstimator(nn.Module):
    """The LMMSE baseline as a module: ``forward(pilot_symbols, meta_data)`` with the six-tuple ``(file_no, snr, ds, dop, n, types)``
    every loader here yields -> complex64 ``[B, S, T]``.  No parameters; the float32 table image is a non-persistent buffer, so
    ``.to(device)`` moves the estimator.  ``assume`` pins conditions (module docstring); with all three pinned ``meta_data`` may be None.

    On a HIP device a forward is ONE launch of ``aft_lmmse_f32`` on the current stream: CPU pilots and CPU conditions are placed in a
    slot of the pinned ring (``estimators._InputStager``) which the kernel reads in place -- no copy is enqueued, nothing is read back,
    nothing synchronises.  On the CPU the float64 definition is evaluated and rounded to complex64."""

    def __init__(self, cfg: ChannelSimConfig, assume=None) -> None:
        super().__init__()
        self.tables = LmmseTables(cfg)
        self.cfg = cfg
        self.assume = _check_assume(assume)
        self.fixed = self.tables.fixed(self.assume)
        self.ofdm_size, self.pilot_size = tuple(cfg.ofdm), tuple(cfg.pilot)
        self.register_buffer("table_image", torch.from_numpy(self.tables.image()), persistent=False)
        self._plan = None
        self._stager = None

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() re-allocate the buffer
        self._plan = None
        return super()._apply(fn, *args, **kwargs)

    def _hip_plan(self):
        img = self.table_image
        if img.dtype != torch.float32:
            raise ValueError(f"the LMMSE table image must stay float32 on the HIP device (it is {img.dtype})")
        if self._plan is None or self._plan.image.data_ptr() != img.data_ptr():
            from .hip_ops import LmmsePlan         # loads the extension: a missing .so raises here, loudly
            self._plan = LmmsePlan(self.tables, img.device, assume=self.assume, image=img)
        return self._plan

    def forward(self, pilot_symbols: torch.Tensor, meta_data: Optional[tuple] = None) -> torch.Tensor:
        if pilot_symbols.dim() != 3 or tuple(pilot_symbols.shape[1:]) != self.pilot_size:
            raise ValueError(f"Expected pilot shape (B, {self.pilot_size[0]}, {self.pilot_size[1]}), got {tuple(pilot_symbols.shape)}")
        if pilot_symbols.dtype != torch.complex64:
            raise ValueError(f"pilot_symbols must be complex64, got {pilot_symbols.dtype}")
        B = pilot_symbols.shape[0]
        conds = None
        if meta_data is not None:
            _, snr, ds, dop, _, _ = meta_data
            conds = [snr, ds, dop]
            if any(c.numel() != B for c in conds):
                raise ValueError("meta_data tensors must have one value per frame")
        elif min(self.fixed) < 0:
            raise ValueError("meta_data is required unless assume pins all three conditions")
        dev = self.table_image.device
        if dev.type != "cuda":
            cond = None if conds is None else np.stack([c.detach().cpu().reshape(-1).double().numpy() for c in conds], axis=1)
            est = lmmse_estimate_host(self.tables, pilot_symbols.detach().cpu().numpy(), cond, self.assume)
            return torch.from_numpy(est.astype(np.complex64))
        if B == 0:
            return torch.empty((0, *self.ofdm_size), dtype=torch.complex64, device=dev)
        plan = self._hip_plan()
        pil_cpu = pilot_symbols.device.type == "cpu"
        cond_cpu = conds is not None and all(c.device.type == "cpu" and c.dtype == torch.float32 for c in conds)
        if conds is not None and not cond_cpu:
            conds = [c.to(device=dev, dtype=torch.float32).reshape(-1).contiguous() for c in conds]
        if not (pil_cpu or cond_cpu):
            return self._launch(plan, pilot_symbols.to(dev), conds)
        from .estimators import _InputStager
        if self._stager is None or self._stager.device != dev:
            self._stager = _InputStager(dev)
        slot, _, pil_h, cond_h = self._stager.fill(pilot_symbols if pil_cpu else None, conds if cond_cpu else None)
        try:
            return self._launch(plan, pil_h if pil_cpu else pilot_symbols.to(dev), cond_h if cond_cpu else conds)
        finally:
            self._stager.release(slot)

    def _launch(self, plan, pilots, conds):
        if torch.cuda.current_device() != plan.device.index:       # the launch belongs to the estimator's device, whichever is current
            with torch.cuda.device(plan.device):
                return plan(pilots, *(conds or (None, None, None)))
        return plan(pilots, *(conds or (None, None, None)))

    def get_model_info(self) -> dict:
        return {"model_name": self.__class__.__name__, "ofdm_size": self.ofdm_size, "pilot_size": self.pilot_size,
                "assume": dict(self.assume), "device": str(self.table_image.device), "total_parameters": 0, "trainable_parameters": 0}
