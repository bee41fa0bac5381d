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

Smoothing and prediction over slot sequences.  On a sequence configuration (``slots = K``, ``slot_symbols = L``, groups of G) the
statistics are known ACROSS slots too -- ``r_t`` at the absolute symbol -- so the best linear estimate of slot ``k`` from the pilots of
the last ``W`` slots up to slot ``k - h`` can be written down as well (``LmmseTables(cfg, window=W, horizon=h)``).  Frame ``(seq, k, a)``,
index ``(seq K + k) G + a``: with ``n = k - h + 1`` the estimate is all zeros when ``n <= 0`` (no observation); otherwise ``w = min(W, n)``
and the observations are member ``a``'s pilots of slots ``k - h - w + 1 .. k - h``, oldest first, side by side along time, ``P [Ps, w Pt]``.
Their symbols sit at ``q_(i,j) = (i - (w - 1) - h) L + sym_j`` relative to the target slot's symbol 0, and::

    R_t^(w) = r_t(q - q') = U_t^(w) diag(lt^(w)) U_t^(w)T     T'^(w) = r_t(t - q) U_t^(w)  [T, w Pt]
    est = F' [ D o (U_f^H P U_t^(w)) ] T'^(w)T,               D[k][l] = 1 / (lf[k] lt^(w)[l] + sigma2)

-- the same Kronecker eigenbasis form with ``w Pt`` for ``Pt``; the frequency tables are untouched and the design point is the TARGET
frame's.  ``lmmse_seq_estimate_host`` is the float64 twin, ``aft_lmmse_seq_f32`` (``hip_ops.LmmseSeqPlan``) the device's one launch per
batch, ``LmmseEstimator(cfg, window=W, horizon=h)`` the module.  ``W = 1, h = 0`` is the single-slot estimator, table for table.

Which design point a frame uses: per condition the index of the NEAREST table value (``|v - value[i]|`` in float64, ties to the lower
index, NaN to index 0) -- a total function, no error path; ``assume=dict(snr_db=.., delay_spread_ns=.., doppler_hz=..)`` pins any of the
three for every frame, whatever its meta says (the mismatched, or robust, receiver); a pinned value is chosen by nearest value too.

Choosing the design point from the pilots.  A receiver has no meta: it has the pilots.  In the eigenbasis above the Gaussian likelihood
of a window's pilots under a design point ``c = (s, d, e) = (i_snr, i_ds, i_dop)`` is diagonal, so the maximum-likelihood design point
is a classification over the ``n_snr n_ds n_dop`` candidates in which no matrix is inverted.  Target frame ``(seq, k, a)`` looks at
exactly what its estimator looks at -- ``w = min(W, k - h + 1)`` slots ending at slot ``k - h``, ``P_a [Ps, w Pt]``, the same tables::

    Z_a = U_f[d]^H P_a U_t^(w)[e]        E_kl = sum_a |Z_a,kl|^2        V_kl = lf[d]_k lt^(w)[e]_l + sigma2[s]
    score(c) = -( m sum_kl log V_kl + sum_kl E_kl / V_kl )

With ``pool=True`` the sum over ``a`` runs over the ``m = G`` members of the frame's group in member order (the simulator defines a
group's conditions as shared) and the group is the UNIT that decides; with ``pool=False`` a frame is its own unit (``m = 1``).  This is
the log-likelihood of the window under a circular Gaussian channel with the simulator's second-order statistics (up to a constant); a
quasi-likelihood here, because a tap is a sum of 8 rays.  The candidate with the highest score wins; ties go to the lowest flat index
``(s n_ds + d) n_dop + e``; a NaN score never wins, and where every score is NaN the choice is index 0 per free condition -- a total
function, like ``nearest_index``.  ``assume`` pins a condition (by nearest value, as above): only candidates with that index compete
(the others' scores read -inf), and with all three pinned nothing is computed.  With ``w = 0`` (``k < h``) there is nothing to look
at: the choice is the pinned index or 0 and the competing scores are 0.  ``lmmse_classify_host`` is the float64 twin,
``aft_lmmse_classify_f32`` (csrc/k_lmmse_classify.hip, through ``hip_ops.LmmseClassifyPlan``) the device's one launch per batch; it
reads the estimator's own image and ONE more table, ``LmmseTables.classify_image()``: float32 ``sum_kl log V_kl`` per ``(d, e, w, s)``
(the device takes no logarithm).  ``ConditionEstimator`` is the module, ``LmmseEstimator(conditions="estimated")`` the blind baseline
(classify, then estimate: two launches, the conditions never leave the device), ``EstimatedConditions`` wraps any estimator with the
``forward(pilot_symbols, meta_data)`` signature and hands it estimated conditions in place of the loader's.

The full-grid smoother.  A receiver that has demodulated a frame holds an observation of the channel at EVERY grid position
(``linksim.link_observe_host``: the received sample divided by the decided symbol at a data element, the noisy pilot at a pilot).  The
best linear estimate from all of them is the form above with "every grid position is a pilot"::

    R_f = r_f(s - s') = U_g diag(lam_g) U_g^H   over all S subcarriers; the Kf = min(S, taps) largest eigenpairs, descending
    R_t = r_t(t - t') = U_tg diag(lam_tg) U_tg^T over all T symbols
    est = F_g [ D o (U_g^H Z U_tg) ] T_g^T,   F_g = U_g diag(lam_g),  T_g = U_tg diag(lam_tg),  D = 1 / (lam_g lam_tg + beta sigma2)

``R_f`` is a sum of one rank-one term per tap, so with ``Kf = min(S, taps)`` nothing is dropped (the largest dropped eigenvalue is
1e-14).  ``beta sigma2`` is ONE noise variance for the whole grid -- the simplification that keeps the estimator Kronecker-separable.
``LmmseTables.grid()`` builds the tables when first asked (``image()``, ``seq_image()`` and ``classify_image()`` do not change),
``lmmse_grid_host`` is the float64 twin, ``lmmse_grid_predicted_mse`` the exact MSE with the sent symbols known,
``aft_lmmse_grid_f32`` (csrc/k_lmmse.hip, through ``hip_ops.LmmseGridPlan``) the device's one launch per batch, and
``linksim.DataAidedRefiner`` the receiver loop that uses it.  ``T`` is at most 32 here.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _abi
from .chansim import ChannelSimConfig

CONDITIONS = ("snr_db", "delay_spread_ns", "doppler_hz")
MAX_WINDOW = 16                                                  # slots a window may span


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


def _check_window(cfg: ChannelSimConfig, window, horizon) -> Tuple[int, int]:
    """(window, horizon) as integers, or the refusal that names the fix."""
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (window, horizon)):
        raise ValueError(f"window = {window!r}, horizon = {horizon!r}: both must be integers")
    W, h, K, Pt = int(window), int(horizon), cfg.slots, cfg.pilot[1]
    if not 1 <= W <= MAX_WINDOW:
        raise ValueError(f"window = {W} is outside 1..{MAX_WINDOW}: choose a window of 1 to {MAX_WINDOW} slots")
    if W * Pt > _abi.AFT_LMMSE_MAX_WINDOW_PILOTS:
        raise ValueError(f"window * Pt = {W} * {Pt} = {W * Pt} pilot symbols exceed the {_abi.AFT_LMMSE_MAX_WINDOW_PILOTS} a window may "
                         f"hold: use window <= {_abi.AFT_LMMSE_MAX_WINDOW_PILOTS // Pt}")
    if (W > 1 or h != 0) and K == 1:
        raise ValueError(f"window = {W}, horizon = {h} need a slot sequence: build the ChannelSimConfig with slots > 1 (it has slots = 1)")
    if not 0 <= h < K:
        raise ValueError(f"horizon = {h} is outside 0..{K - 1}: a prediction looks at most slots - 1 = {K - 1} slots ahead")
    return W, h


class LmmseTables:
    """The estimator's tables for one ``ChannelSimConfig``: float64 (``sigma2 [n_snr]``; per delay spread ``lam_f [Ps]``, ``u_f
    [Ps, Ps]``, ``f [S, Ps]`` = F'; per Doppler ``lam_t [Pt]``, ``u_t [Pt, Pt]``, ``t [T, Pt]`` = T') and ``image()``, the float32
    array ``aft_lmmse_f32`` reads (include/adafortitran_amd.h documents its layout).  With ``window > 1`` or ``horizon > 0`` (module
    docstring; the config must have ``slots > 1``) it also holds, per Doppler, the lists ``lam_t_w``, ``u_t_w``, ``t_w`` over
    ``w = 1 .. window`` (entry ``w - 1``: ``[w Pt]``, ``[w Pt, w Pt]``, ``[T, w Pt]``), and ``seq_image()`` is what ``aft_lmmse_seq_f32``
    reads.  The defaults leave the object and ``image()`` as they are without the two keywords."""

    def __init__(self, cfg: ChannelSimConfig, window: int = 1, horizon: int = 0) -> None:
        if not isinstance(cfg, ChannelSimConfig):
            raise ValueError(f"LmmseTables needs a chansim.ChannelSimConfig (got {type(cfg).__name__})")
        self.cfg = cfg
        self.window, self.horizon = _check_window(cfg, window, horizon)
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
        if self.multi_slot:                                      # per Doppler the lists over w = 1 .. W (entry w - 1)
            self.lam_t_w, self.u_t_w, self.t_w = [], [], []
            for i in range(len(self.doppler_turns)):
                lams, us, ts = [], [], []
                for w in range(1, self.window + 1):
                    q = self.window_symbols(w)
                    lam, u = np.linalg.eigh(self.r_t(q[:, None] - q[None, :], i))
                    lams.append(np.maximum(lam, 0.0))
                    us.append(u)
                    ts.append(self.r_t(np.arange(T)[:, None] - q[None, :], i) @ u)
                self.lam_t_w.append(lams)
                self.u_t_w.append(us)
                self.t_w.append(ts)

        self._grid = None                                        # the full-grid tables, built when first asked for

    @property
    def multi_slot(self) -> bool:
        return self.window > 1 or self.horizon > 0

    def grid(self) -> "GridTables":
        """The full-grid smoother's tables (module docstring, "the full-grid smoother"), built on first use and kept: ``image()``,
        ``seq_image()`` and ``classify_image()`` do not see them."""
        if self._grid is None:
            self._grid = GridTables(self)
        return self._grid

    def window_symbols(self, w: int) -> np.ndarray:
        """The ``w Pt`` pilot symbols of a window of ``w`` slots that ends ``horizon`` slots before the target slot, relative to the
        target slot's symbol 0, oldest first: ``(i - (w - 1) - horizon) L + sym_j``."""
        slot = (np.arange(w) - (w - 1) - self.horizon) * self.cfg.slot_symbols
        return (slot[:, None] + self.sym[None, :]).reshape(-1)

    def slot_window(self, k) -> np.ndarray:
        """``w`` of slot ``k``: ``min(window, k - horizon + 1)``, 0 where there is nothing to look at."""
        return np.clip(np.asarray(k, dtype=np.int64) - self.horizon + 1, 0, self.window)

    def time(self, i_dop: int, w: int):
        """``(lt^(w) [w Pt], U_t^(w) [w Pt, w Pt], T'^(w) [T, w Pt])`` of a Doppler."""
        if not 1 <= w <= self.window:
            raise ValueError(f"w = {w} is outside 1..{self.window}, the window these tables were built for")
        if not self.multi_slot:
            return self.lam_t[i_dop], self.u_t[i_dop], self.t[i_dop]
        return self.lam_t_w[i_dop][w - 1], self.u_t_w[i_dop][w - 1], self.t_w[i_dop][w - 1]

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

    def gain(self, i_snr: int, i_ds: int, i_dop: int, w: Optional[int] = None) -> np.ndarray:
        """D [Ps, Pt] of a design point; with ``w`` the window's, [Ps, w Pt]."""
        lam_t = self.lam_t[i_dop] if w is None else self.time(i_dop, w)[0]
        return 1.0 / (self.lam_f[i_ds][:, None] * lam_t[None, :] + self.sigma2[i_snr])

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

    def seq_image(self) -> np.ndarray:
        """The float32 table image of ``aft_lmmse_seq_f32``: the frequency blocks of ``image()``, then per Doppler the ``window``
        sub-blocks ``U_t^(w)``, ``T'^(w)`` (l-major), ``lt^(w)`` for ``w = 1 .. window``.  With ``window = 1, horizon = 0`` it is ``image()``."""
        Ps = self.cfg.pilot[0]
        pairs = lambda z: np.stack([z.real, z.imag], axis=-1).reshape(-1)  # noqa: E731
        parts = []
        for lam, u, f in zip(self.lam_f, self.u_f, self.f):
            parts += [pairs(u.conj().T), pairs(f.T), lam, np.zeros(Ps & 1)]
        for i in range(len(self.doppler_turns)):
            for w in range(1, self.window + 1):
                lam, u, t = self.time(i, w)
                parts += [u.reshape(-1), t.T.reshape(-1), lam]
        return np.concatenate(parts).astype(np.float32)

    def logdet(self, i_ds: int, i_dop: int, w: int) -> np.ndarray:
        """``sum_kl log(lf[k] lt^(w)[l] + sigma2[s])`` for every SNR of the table (float64 ``[n_snr]``)."""
        lam = self.lam_f[i_ds][:, None] * self.time(i_dop, w)[0][None, :]
        return np.log(lam[None] + self.sigma2[:, None, None]).sum(axis=(1, 2))

    def classify_image(self) -> np.ndarray:
        """The float32 table ``aft_lmmse_classify_f32`` reads beside ``seq_image()`` / ``image()``: ``logdet`` as
        ``[n_ds][n_dop][window][n_snr]`` (entry ``w - 1`` for a window of ``w`` slots)."""
        out = [self.logdet(d, e, w) for d in range(len(self.delay_turns)) for e in range(len(self.doppler_turns))
               for w in range(1, self.window + 1)]
        return np.concatenate(out).astype(np.float32)

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


MAX_GRID_SYMBOLS = _abi.AFT_LMMSE_MAX_WINDOW_PILOTS              # symbols the full-grid smoother filters at once


class GridTables:
    """The full-grid smoother's tables for the config of ``tables`` (module docstring, "the full-grid smoother"; ``LmmseTables.grid()``
    builds them once): float64, per delay spread ``lam_g [Kf]`` (descending, clamped at 0) and ``u_g [S, Kf]``, the ``Kf = min(S, taps)``
    largest eigenpairs of ``r_f`` over all ``S`` subcarriers; per Doppler ``lam_tg [T]`` and ``u_tg [T, T]`` of ``r_t`` over all ``T``
    symbols.  ``image()`` is the float32 array ``aft_lmmse_grid_f32`` reads (include/adafortitran_amd.h documents its layout)."""

    def __init__(self, tables: LmmseTables) -> None:
        S, T = tables.cfg.ofdm
        if T > MAX_GRID_SYMBOLS:
            raise ValueError(f"ofdm grid {S} x {T}: the full-grid smoother filters all T symbols of a frame at once and holds at most "
                             f"{MAX_GRID_SYMBOLS} of them (T > {MAX_GRID_SYMBOLS} is out of its scope); the pilot estimator "
                             f"LmmseEstimator takes any T")
        self.tables = tables
        self.kf = Kf = min(S, len(tables.pw))
        s, t = np.arange(S), np.arange(T)
        self.lam_g, self.u_g = [], []
        for i in range(len(tables.delay_turns)):
            lam, u = np.linalg.eigh(tables.r_f(s[:, None] - s[None, :], i))
            self.lam_g.append(np.maximum(lam[::-1][:Kf], 0.0))
            self.u_g.append(np.ascontiguousarray(u[:, ::-1][:, :Kf]))
        self.lam_tg, self.u_tg = [], []
        for i in range(len(tables.doppler_turns)):
            lam, u = np.linalg.eigh(tables.r_t(t[:, None] - t[None, :], i))
            self.lam_tg.append(np.maximum(lam, 0.0))
            self.u_tg.append(u)

    def noise(self, noise_scale: float = 1.0) -> np.ndarray:
        """``noise_scale * sigma2`` per SNR value, float64 ``[n_snr]``."""
        beta = float(noise_scale)
        if not (np.isfinite(beta) and beta > 0.0):
            raise ValueError(f"noise_scale = {noise_scale!r}: a finite positive factor on the noise variance")
        return beta * self.tables.sigma2

    def gain(self, i_snr: int, i_ds: int, i_dop: int, noise_scale: float = 1.0) -> np.ndarray:
        """D [Kf, T] of a design point."""
        return 1.0 / (self.lam_g[i_ds][:, None] * self.lam_tg[i_dop][None, :] + self.noise(noise_scale)[i_snr])

    def image(self) -> np.ndarray:
        pairs = lambda z: np.stack([z.real, z.imag], axis=-1).reshape(-1)  # noqa: E731
        parts = []
        for lam, u in zip(self.lam_g, self.u_g):
            parts += [pairs(u.conj()), pairs((u * lam[None, :]).T), lam, np.zeros(self.kf & 1)]
        for lam, u in zip(self.lam_tg, self.u_tg):
            parts += [u.reshape(-1), (u * lam[None, :]).T.reshape(-1), lam]
        return np.concatenate(parts).astype(np.float32)

    def to_struct(self, assume=None, noise_scale: float = 1.0) -> "_abi.AftLmmse":
        """The estimator's struct with ``noise_var[i] = float32(noise_scale * sigma2[i])``: formed in double, rounded once."""
        p = self.tables.to_struct(assume)
        for i, v in enumerate(self.noise(noise_scale).astype(np.float32)):
            p.noise_var[i] = float(v)
        return p


def lmmse_grid_host(tables: Union[ChannelSimConfig, LmmseTables], z, conditions, assume=None, noise_scale: float = 1.0) -> np.ndarray:
    """The full-grid smoother in float64 (module docstring, "the full-grid smoother"): observations ``z [n, S, T]`` of every grid
    position and conditions ``[n, 3]`` -> complex128 ``[n, S, T]``, ``est = F_g [ D o (U_g^H Z U_tg) ] T_g^T`` with ``D = 1 / (lam_g
    lam_tg + noise_scale sigma2[i_snr])``.  THE SIMPLIFICATION: one noise variance ``noise_scale * sigma2`` for the whole grid,
    although a decision-directed observation carries ``sigma2`` at a pilot and ``sigma2 / |x|^2`` at a data element
    (``linksim.data_noise_scale(m)`` is the data elements' average factor); the estimator stays linear and Kronecker-separable, and
    ``lmmse_grid_predicted_mse`` says what that costs.  The design point is ``indices()``'s, as everywhere.  Needs no library."""
    tb = _tables(tables)
    g = tb.grid()
    z = np.asarray(z).astype(np.complex128)
    if z.ndim != 3 or z.shape[1:] != tuple(tb.cfg.ofdm):
        raise ValueError(f"Expected observations of shape (n, {tb.cfg.ofdm[0]}, {tb.cfg.ofdm[1]}), got {z.shape}")
    if conditions is None:
        if min(tb.fixed(assume)) < 0:
            raise ValueError("conditions are required unless assume pins all three")
        conditions = np.zeros((len(z), 3))
    i_snr, i_ds, i_dop = tb.indices(conditions, assume)
    if len(i_snr) != len(z):
        raise ValueError(f"{len(z)} frames but {len(i_snr)} rows of conditions")
    out = np.empty(z.shape, dtype=np.complex128)
    key = i_snr * 1024 + i_ds * 32 + i_dop
    for k in np.unique(key):
        sel = np.nonzero(key == k)[0]
        a, d, e = int(i_snr[sel[0]]), int(i_ds[sel[0]]), int(i_dop[sel[0]])
        y = np.einsum("sk,nst,tl->nkl", g.u_g[d].conj(), z[sel], g.u_tg[e]) * g.gain(a, d, e, noise_scale)[None]
        out[sel] = np.einsum("sk,nkl,tl->nst", g.u_g[d] * g.lam_g[d][None, :], y, g.u_tg[e] * g.lam_tg[e][None, :])
    return out


def lmmse_grid_predicted_mse(tables: Union[ChannelSimConfig, LmmseTables], snr_db: float, delay_spread_ns: float, doppler_hz: float,
                             m: int) -> float:
    """The exact MSE per grid element of ``lmmse_grid_host(noise_scale=data_noise_scale(m))`` on the observations of
    ``linksim.link_observe_host(source="sent")`` with ``m`` bits per symbol, at the given condition (its nearest table values).  The
    estimator is ``W = Q diag(g) Q^H`` with ``Q = U_g (x) U_tg`` and ``g_kl = lam_kl / (lam_kl + beta sigma2)``; the channel's
    covariance is ``Q diag(lam) Q^H`` and the noise is independent with a DIAGONAL covariance, ``n_i = sigma2`` at a pilot and
    ``beta sigma2`` on average at a data element (``beta = data_noise_scale(m)``, the mean of ``1 / |x|^2``), so
    ``MSE = (1 / ST) [ sum_kl lam_kl (1 - g_kl)^2 + sum_i n_i |W[:, i]|^2 ]`` and the noise term separates over the Kronecker factors:
    ``sum_i n_i |W[:, i]|^2 = beta sigma2 sum_kl g_kl^2 - (beta - 1) sigma2 sum_kl g_kl^2 A_k B_l`` with ``A_k = sum_{s in sc}
    |U_g[s, k]|^2`` and ``B_l = sum_{t in sym} U_tg[t, l]^2`` the eigenvectors' mass at the pilot rows and columns."""
    from .linksim import data_noise_scale
    tb = _tables(tables)
    g = tb.grid()
    a, d, e = (int(v[0]) for v in tb.indices([[snr_db, delay_spread_ns, doppler_hz]]))
    beta, s2 = data_noise_scale(m), float(tb.sigma2[a])
    S, T = tb.cfg.ofdm
    lam = g.lam_g[d][:, None] * g.lam_tg[e][None, :]
    gain = lam / (lam + beta * s2)
    at_sc = (np.abs(g.u_g[d][tb.sc]) ** 2).sum(axis=0)
    at_sym = (g.u_tg[e][tb.sym] ** 2).sum(axis=0)
    noise = beta * s2 * (gain ** 2).sum() - (beta - 1.0) * s2 * float(at_sc @ (gain ** 2) @ at_sym)
    return float(((lam * (1.0 - gain) ** 2).sum() + noise) / (S * T))


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


def _seq_tables(tables: Union[ChannelSimConfig, LmmseTables], window, horizon) -> LmmseTables:
    """The tables a multi-slot call works with: ``tables`` itself when ``window`` / ``horizon`` (None: its own) fit it."""
    if not isinstance(tables, LmmseTables):
        return LmmseTables(tables, 1 if window is None else window, 0 if horizon is None else horizon)
    W, h = tables.window if window is None else window, tables.horizon if horizon is None else horizon
    if h == tables.horizon and 1 <= W <= tables.window:          # a shorter window of the same horizon is among its lists
        return tables
    return LmmseTables(tables.cfg, W, h)


def lmmse_seq_estimate_host(tables: Union[ChannelSimConfig, LmmseTables], pilots, conditions, assume=None) -> np.ndarray:
    """The multi-slot definition in float64 (module docstring): pilots ``[n, Ps, Pt]`` of whole sequences in order (``n`` a multiple of
    ``K G``) and conditions ``[n, 3]`` -> complex128 ``[n, S, T]``.  Window and horizon are the tables' (``LmmseTables(cfg, window,
    horizon)``; a bare config means 1 and 0, the single-slot estimator).  A frame's design point comes from its OWN row of
    ``conditions``.  Needs no library."""
    tb = _tables(tables)
    cfg = tb.cfg
    pilots = np.asarray(pilots).astype(np.complex128)
    if pilots.ndim != 3 or pilots.shape[1:] != tuple(cfg.pilot):
        raise ValueError(f"Expected pilot shape (n, {cfg.pilot[0]}, {cfg.pilot[1]}), got {pilots.shape}")
    K, G, n = cfg.slots, cfg.group, len(pilots)
    if n % (K * G):
        raise ValueError(f"{n} frames are not whole sequences: pass a multiple of slots * group = {K} * {G} = {K * G} frames, in "
                         f"sequence order")
    if conditions is None:
        if min(tb.fixed(assume)) < 0:
            raise ValueError("conditions are required unless assume pins all three")
        conditions = np.zeros((n, 3))
    i_snr, i_ds, i_dop = tb.indices(conditions, assume)
    if len(i_snr) != n:
        raise ValueError(f"{n} frames but {len(i_snr)} rows of conditions")
    Ps, Pt = cfg.pilot
    out = np.zeros((n, *cfg.ofdm), dtype=np.complex128)
    frame = np.arange(n)
    ws = tb.slot_window(frame // G % K)
    key = (i_snr * 1024 + i_ds * 32 + i_dop) * 64 + ws
    for k in np.unique(key[ws > 0]):
        sel = np.nonzero(key == k)[0]
        a, d, e, w = int(i_snr[sel[0]]), int(i_ds[sel[0]]), int(i_dop[sel[0]]), int(ws[sel[0]])
        _, u_t, t = tb.time(e, w)
        src = sel[:, None] - (tb.horizon + w - 1 - np.arange(w))[None, :] * G                 # [m, w], oldest first
        p = pilots[src].transpose(0, 2, 1, 3).reshape(len(sel), Ps, w * Pt) if w > 1 or tb.horizon else pilots[sel]
        y = np.einsum("ik,nij,jl->nkl", tb.u_f[d].conj(), p, u_t) * tb.gain(a, d, e, w)[None]
        out[sel] = np.einsum("sk,nkl,tl->nst", tb.f[d], y, t)
    return out


def _classify_units(tb: LmmseTables, n: int, pool: bool) -> Tuple[int, int, int]:
    """(K, G, m) a classification of ``n`` frames works with: slots per sequence and frames per slot as far as they matter (single-slot
    tables look at no other slot, a frame that decides alone at no other member), members per unit; or the refusal that names the fix."""
    K = tb.cfg.slots if tb.multi_slot else 1
    G = tb.cfg.group if (tb.multi_slot or pool) else 1
    if n % (K * G):
        if K > 1:
            raise ValueError(f"{n} frames are not whole sequences: pass a multiple of slots * group = {K} * {G} = {K * G} frames, in "
                             f"sequence order")
        raise ValueError(f"{n} frames are not whole groups: pass a multiple of group = {G} frames, in group order, or pool=False to "
                         f"let every frame decide alone")
    return K, G, (G if pool else 1)


def lmmse_classify_host(tables: Union[ChannelSimConfig, LmmseTables], pilots, assume=None, pool: bool = True, return_scores: bool = False):
    """The design point from the pilots, in float64 (module docstring, "choosing the design point from the pilots"): pilots
    ``[n, Ps, Pt]`` of whole sequences in order -> ``(idx int64 [n, 3], values float32 [n, 3])``, the chosen ``(i_snr, i_ds, i_dop)`` and
    the table values ``(snr_db, delay_spread_ns, doppler_hz)`` in the form ``meta`` has; with ``return_scores`` also the scores, float64
    ``[units, n_snr n_ds n_dop]`` in flat index order, a unit being a group (``pool=True``) or a frame.  Window and horizon are the tables'
    (a bare config or single-slot tables: 1 and 0, and then any number of whole groups -- of frames with ``pool=False`` -- will do).
    Needs no library."""
    tb = _tables(tables)
    cfg = tb.cfg
    pilots = np.asarray(pilots).astype(np.complex128)
    if pilots.ndim != 3 or pilots.shape[1:] != tuple(cfg.pilot):
        raise ValueError(f"Expected pilot shape (n, {cfg.pilot[0]}, {cfg.pilot[1]}), got {pilots.shape}")
    if not isinstance(pool, (bool, np.bool_)):
        raise ValueError(f"pool must be True (a group decides together) or False (every frame alone); got {pool!r}")
    n = len(pilots)
    K, G, m = _classify_units(tb, n, bool(pool))
    Ps, Pt = cfg.pilot
    fixed = tb.fixed(assume)
    sizes = tuple(len(tb.values[name]) for name in CONDITIONS)
    n_snr, n_ds, n_dop = sizes
    compete = np.ones(sizes, dtype=bool)
    for axis, f in enumerate(fixed):
        if f >= 0:
            keep = np.zeros(sizes[axis], dtype=bool)
            keep[f] = True
            compete &= keep.reshape([-1 if a == axis else 1 for a in range(3)])
    lowest = int(np.flatnonzero(compete.reshape(-1))[0])                                       # the pinned index or 0 per condition
    units = n // m
    head = np.arange(units) * m                                                                # a unit's first frame
    ws = tb.slot_window(head // G % K)
    scores = np.where(compete.reshape(-1), 0.0, -np.inf)[None, :].repeat(units, axis=0)
    if min(fixed) < 0:                                                                         # all three pinned: nothing is computed
        for w in np.unique(ws[ws > 0]):
            w = int(w)
            sel = np.nonzero(ws == w)[0]
            frames = head[sel][:, None] + np.arange(m)[None, :]                                # [u, m]
            src = frames[:, :, None] - (tb.horizon + w - 1 - np.arange(w))[None, None, :] * G  # [u, m, w], oldest first
            p = pilots[src].transpose(0, 1, 3, 2, 4).reshape(len(sel), m, Ps, w * Pt)
            for d in range(n_ds):
                if fixed[1] >= 0 and d != fixed[1]:
                    continue
                y1 = np.einsum("ik,umij->umkj", tb.u_f[d].conj(), p)
                for e in range(n_dop):
                    if fixed[2] >= 0 and e != fixed[2]:
                        continue
                    lam_t, u_t, _ = tb.time(e, w)
                    energy = (np.abs(np.einsum("umkj,jl->umkl", y1, u_t)) ** 2).sum(axis=1)   # E [u, Ps, w Pt]: over members first
                    v = (tb.lam_f[d][:, None] * lam_t[None, :])[None] + tb.sigma2[:, None, None]
                    with np.errstate(invalid="ignore", over="ignore"):
                        q = np.einsum("ukl,skl->us", energy, 1.0 / v)
                        sc = -(m * tb.logdet(d, e, w)[None, :] + q)                           # [u, n_snr]
                    for s in range(n_snr):
                        if fixed[0] < 0 or s == fixed[0]:
                            scores[sel, (s * n_ds + d) * n_dop + e] = sc[:, s]
    ranked = np.where(np.isnan(scores), -np.inf, scores)
    pick = ranked.argmax(axis=1)                                                               # the first of the highest: the lowest index
    pick = np.where(np.isneginf(ranked.max(axis=1)), lowest, pick)
    idx_u = np.stack([pick // (n_ds * n_dop), pick // n_dop % n_ds, pick % n_dop], axis=1).astype(np.int64)
    idx = np.repeat(idx_u, m, axis=0)
    values = np.stack([tb.values[name][idx[:, k]] for k, name in enumerate(CONDITIONS)], axis=1).astype(np.float32)
    return (idx, values, scores) if return_scores else (idx, values)


def lmmse_predicted_mse(cfg: Union[ChannelSimConfig, LmmseTables], snr_db: float, delay_spread_ns: float, doppler_hz: float,
                        assume=None, window: Optional[int] = None, horizon: Optional[int] = None, slot: Optional[int] = None) -> float:
    """The closed-form MSE per grid element of the estimator on frames drawn at the given condition (its nearest table values).
    Matched: ``1 - (1 / ST) sum_{s,t} sum_{k,l} |F'_sk|^2 T'_tl^2 D_kl``.  With ``assume`` the estimator ``W`` is that of the pinned
    design while the statistics are the true ones: ``1 - 2 Re diag(W R_ph) + diag(W (R_pp + sigma2 I) W^H)``, averaged over the grid
    (full matrices: host only).
    ``window`` / ``horizon`` (None: the tables' own, 1 and 0 for a config): the multi-slot estimator's MSE on a slot with a FULL
    window -- the same expressions over ``T'^(W)`` and over the window's pilot set.  ``slot=k`` gives slot k's value instead, with its
    shorter window ``w = min(W, k - h + 1)`` early in a sequence, and 1.0 (``E|H|^2``) where there is nothing to look at."""
    tb = _seq_tables(cfg, window, horizon)
    w = int(tb.window if window is None else window)
    if slot is not None:
        if not 0 <= int(slot) < tb.cfg.slots:
            raise ValueError(f"slot = {slot} is outside 0..{tb.cfg.slots - 1}")
        w = int(min(w, int(slot) - tb.horizon + 1))
        if w <= 0:
            return 1.0
    true = tuple(int(v[0]) for v in tb.indices([[snr_db, delay_spread_ns, doppler_hz]]))
    used = tuple(int(v[0]) for v in tb.indices([[snr_db, delay_spread_ns, doppler_hz]], assume))
    S, T = tb.cfg.ofdm
    if used == true:
        a, d, e = true
        return float(1.0 - np.einsum("sk,tl,kl->", np.abs(tb.f[d]) ** 2, tb.time(e, w)[2] ** 2, tb.gain(a, d, e, w)) / (S * T))
    a, d, e = used
    _, u_t, t_p = tb.time(e, w)
    w_mat = (np.kron(tb.f[d], t_p) * tb.gain(a, d, e, w).reshape(-1)[None, :]) @ np.kron(tb.u_f[d], u_t).conj().T          # [ST, Ps wPt]
    a, d, e = true
    s, t, q = np.arange(S), np.arange(T), tb.window_symbols(w)
    r_ph = np.kron(tb.r_f(tb.sc[:, None] - s[None, :], d), tb.r_t(q[:, None] - t[None, :], e))                             # [Ps wPt, ST]
    r_pp = np.kron(tb.r_f(tb.sc[:, None] - tb.sc[None, :], d), tb.r_t(q[:, None] - q[None, :], e))
    r_pp = r_pp + tb.sigma2[a] * np.eye(len(r_pp))
    per = 1.0 - 2.0 * np.real((w_mat * r_ph.T).sum(axis=1)) + np.real(((w_mat @ r_pp) * w_mat.conj()).sum(axis=1))
    return float(per.mean())


class LmmseEstimator(nn.Module):
    """The LMMSE baseline as a module: ``forward(pilot_symbols, meta_data)`` with the six-tuple ``(file_no, snr, ds, dop, n, types)``
    every loader here yields -> complex64 ``[B, S, T]``.  No parameters; the float32 table image is a non-persistent buffer, so
    ``.to(device)`` moves the estimator.  ``assume`` pins conditions (module docstring); with all three pinned ``meta_data`` may be None.

    On a HIP device a forward is ONE launch of ``aft_lmmse_f32`` on the current stream: CPU pilots and CPU conditions are placed in a
    slot of the pinned ring (``estimators._InputStager``) which the kernel reads in place -- no copy is enqueued, nothing is read back,
    nothing synchronises.  On the CPU the float64 definition is evaluated and rounded to complex64.

    ``window=W`` / ``horizon=h`` (module docstring, "smoothing and prediction over slot sequences"; the defaults are the single-slot
    estimator, launch for launch): slot k of every sequence is estimated from the pilots of the last W slots up to slot k - h.  A batch
    must then hold WHOLE sequences in order (``B`` a multiple of ``slots * group``), as ``SynthLoader``, ``make_pack`` and an unshuffled
    ``ResidentLoader`` deliver them; the forward is one launch of ``aft_lmmse_seq_f32`` through the same pinned ring, and on the CPU
    ``lmmse_seq_estimate_host``.

    ``conditions="estimated"`` is the BLIND baseline (module docstring, "choosing the design point from the pilots"; the default
    ``"meta"`` is the module above, launch for launch): the three condition entries of ``meta_data`` are ignored (it may be None) and the
    design point is the maximum-likelihood one of the frame's own window, pooled over its group with ``pool=True``.  On a HIP device that
    is two launches, ``aft_lmmse_classify_f32`` then the estimator, and the conditions never leave the device; ``assume`` pins conditions
    for both.  A batch then holds whole groups (whole sequences with a window), as the classification needs them."""

    def __init__(self, cfg: ChannelSimConfig, assume=None, window: int = 1, horizon: int = 0, conditions: str = "meta",
                 pool: bool = True) -> None:
        super().__init__()
        if conditions not in ("meta", "estimated"):
            raise ValueError(f'conditions = {conditions!r}: choose "meta" (the loader\'s conditions) or "estimated" (chosen from the pilots)')
        self.conditions = conditions
        self.chooser = ConditionEstimator(cfg, window, horizon, assume, pool) if conditions == "estimated" else None
        self.tables = LmmseTables(cfg, window, horizon) if self.chooser is None else self.chooser.tables
        self.window, self.horizon = self.tables.window, self.tables.horizon
        self.cfg = cfg
        self.assume = _check_assume(assume)
        self.fixed = self.tables.fixed(self.assume)
        self.ofdm_size, self.pilot_size = tuple(cfg.ofdm), tuple(cfg.pilot)
        if self.chooser is None:
            image = torch.from_numpy(self.tables.seq_image() if self.tables.multi_slot else self.tables.image())
        else:
            image = self.chooser.table_image                         # the same image: ONE tensor serves both launches
        self.register_buffer("table_image", image, persistent=False)
        self._plan = None
        self._stager = None

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() re-allocate the buffer
        self._plan = None
        out = super()._apply(fn, *args, **kwargs)
        if self.chooser is not None:                # ... each module its own: keep the chooser's, drop the copy
            self._buffers["table_image"] = self.chooser.table_image
        return out

    def _hip_plan(self):
        img = self.table_image
        if img.dtype != torch.float32:
            raise ValueError(f"the LMMSE table image must stay float32 on the HIP device (it is {img.dtype})")
        if self._plan is None or self._plan.image.data_ptr() != img.data_ptr():
            from .hip_ops import LmmsePlan, LmmseSeqPlan   # loads the extension: a missing .so raises here, loudly
            plan = LmmseSeqPlan if self.tables.multi_slot else LmmsePlan
            self._plan = plan(self.tables, img.device, assume=self.assume, image=img)
        return self._plan

    def steady_slots(self) -> range:
        """``range(W - 1 + h, K)``: the slots of a sequence whose window is full.  The evaluation sweep (``evaluation.get_test_stats``)
        averages over ALL slots, the warm-up slots before these included (their shorter windows, and the all-zero estimates of the first
        ``h`` slots, whose error is ``|H|^2``); a per-slot figure has to select these slots itself."""
        return range(self.window - 1 + self.horizon, self.cfg.slots)

    def forward(self, pilot_symbols: torch.Tensor, meta_data: Optional[tuple] = None) -> torch.Tensor:
        if pilot_symbols.dim() != 3 or tuple(pilot_symbols.shape[1:]) != self.pilot_size:
            raise ValueError(f"Expected pilot shape (B, {self.pilot_size[0]}, {self.pilot_size[1]}), got {tuple(pilot_symbols.shape)}")
        if pilot_symbols.dtype != torch.complex64:
            raise ValueError(f"pilot_symbols must be complex64, got {pilot_symbols.dtype}")
        B = pilot_symbols.shape[0]
        unit = self.cfg.sequence()
        if self.tables.multi_slot and B % unit:
            raise ValueError(f"window = {self.window}, horizon = {self.horizon} need whole sequences in order: the batch of {B} frames "
                             f"is not a multiple of slots * group = {self.cfg.slots} * {self.cfg.group} = {unit}")
        conds = None
        estimated = self.chooser is not None
        if estimated:
            _classify_units(self.tables, B, self.chooser.pool)
        elif meta_data is not None:
            _, snr, ds, dop, _, _ = meta_data
            conds = [snr, ds, dop]
            if any(c.numel() != B for c in conds):
                raise ValueError("meta_data tensors must have one value per frame")
        elif min(self.fixed) < 0:
            raise ValueError("meta_data is required unless assume pins all three conditions")
        dev = self.table_image.device
        if dev.type != "cuda":
            cond = None if conds is None else np.stack([c.detach().cpu().reshape(-1).double().numpy() for c in conds], axis=1)
            if estimated:
                cond = lmmse_classify_host(self.tables, pilot_symbols.detach().cpu().numpy(), self.assume, self.chooser.pool)[1]
            host = lmmse_seq_estimate_host if self.tables.multi_slot else lmmse_estimate_host
            est = host(self.tables, pilot_symbols.detach().cpu().numpy(), cond, self.assume)
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
                return self._launch(plan, pilots, conds)
        if self.chooser is not None and min(self.fixed) < 0:        # classify, then estimate: the same pilots, where they are
            conds = self.chooser.hip_plan()(pilots)[1:4]
        return plan(pilots, *(conds or (None, None, None)))

    def get_model_info(self) -> dict:
        return {"model_name": self.__class__.__name__, "ofdm_size": self.ofdm_size, "pilot_size": self.pilot_size,
                "assume": dict(self.assume), "window": self.window, "horizon": self.horizon, "conditions": self.conditions, "device": str(self.table_image.device), "total_parameters": 0, "trainable_parameters": 0}


class ConditionEstimator(nn.Module):
    """The design point from the pilots as a module (module docstring, "choosing the design point from the pilots"):
    ``forward(pilot_symbols)`` with complex64 ``[B, Ps, Pt]`` -> ``(snr, ds, dop)``, float32 ``[B]`` each, the table values of the
    maximum-likelihood candidate of every frame's window (``window`` / ``horizon`` as ``LmmseEstimator``'s; ``pool``: a group decides
    together); ``classify(pilot_symbols, scores=False)`` also returns the indices, ``(idx [B, 3], snr, ds, dop[, scores])``.  No
    parameters; the two float32 tables are non-persistent buffers.  On a HIP device a forward is ONE launch of
    ``aft_lmmse_classify_f32`` on the current stream (``hip_ops.LmmseClassifyPlan``), CPU pilots going through the pinned ring of
    ``LmmseEstimator``: nothing is copied, read back or synchronised, and idx is int32.  On the CPU it is ``lmmse_classify_host``
    (idx int64).  A batch holds whole groups when pooling, whole sequences with a window."""

    def __init__(self, cfg: ChannelSimConfig, window: int = 1, horizon: int = 0, assume=None, pool: bool = True) -> None:
        super().__init__()
        if not isinstance(pool, (bool, np.bool_)):
            raise ValueError(f"pool must be True (a group decides together) or False (every frame alone); got {pool!r}")
        self.tables = LmmseTables(cfg, window, horizon)
        self.cfg, self.window, self.horizon, self.pool = cfg, self.tables.window, self.tables.horizon, bool(pool)
        self.assume = _check_assume(assume)
        self.fixed = self.tables.fixed(self.assume)
        self.pilot_size = tuple(cfg.pilot)
        image = self.tables.seq_image() if self.tables.multi_slot else self.tables.image()
        self.register_buffer("table_image", torch.from_numpy(image), persistent=False)
        self.register_buffer("logdet_image", torch.from_numpy(self.tables.classify_image()), persistent=False)
        self._plan = None
        self._stager = None

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() re-allocate the buffers
        self._plan = None
        return super()._apply(fn, *args, **kwargs)

    def hip_plan(self):
        img, ld = self.table_image, self.logdet_image
        if img.dtype != torch.float32 or ld.dtype != torch.float32:
            raise ValueError(f"the classification tables must stay float32 on the HIP device (they are {img.dtype}, {ld.dtype})")
        if self._plan is None or self._plan.image.data_ptr() != img.data_ptr() or self._plan.logdet.data_ptr() != ld.data_ptr():
            from .hip_ops import LmmseClassifyPlan       # loads the extension: a missing .so raises here, loudly
            self._plan = LmmseClassifyPlan(self.tables, img.device, assume=self.assume, pool=self.pool, image=img, logdet=ld)
        return self._plan

    def classify(self, pilot_symbols: torch.Tensor, scores: bool = False):
        if pilot_symbols.dim() != 3 or tuple(pilot_symbols.shape[1:]) != self.pilot_size:
            raise ValueError(f"Expected pilot shape (B, {self.pilot_size[0]}, {self.pilot_size[1]}), got {tuple(pilot_symbols.shape)}")
        if pilot_symbols.dtype != torch.complex64:
            raise ValueError(f"pilot_symbols must be complex64, got {pilot_symbols.dtype}")
        B = pilot_symbols.shape[0]
        _, _, m = _classify_units(self.tables, B, self.pool)
        dev = self.table_image.device
        if dev.type != "cuda":
            out = lmmse_classify_host(self.tables, pilot_symbols.detach().cpu().numpy(), self.assume, self.pool, return_scores=scores)
            res = (torch.from_numpy(out[0]), *(torch.from_numpy(np.ascontiguousarray(out[1][:, k])) for k in range(3)))
            return res + (torch.from_numpy(out[2]),) if scores else res
        if B == 0:
            res = (torch.empty((0, 3), dtype=torch.int32, device=dev), *(torch.empty(0, dtype=torch.float32, device=dev) for _ in range(3)))
            return res + (torch.empty((0, self.logdet_image.numel() // self.window), dtype=torch.float32, device=dev),) if scores else res
        plan = self.hip_plan()
        if pilot_symbols.device.type != "cpu":
            return self._launch(plan, pilot_symbols.to(dev), scores)
        from .estimators import _InputStager
        if self._stager is None or self._stager.device != dev:
            self._stager = _InputStager(dev)
        slot, _, pil_h, _ = self._stager.fill(pilot_symbols, None)
        try:
            return self._launch(plan, pil_h, scores)
        finally:
            self._stager.release(slot)

    def _launch(self, plan, pilots, scores):
        if torch.cuda.current_device() != plan.device.index:       # the launch belongs to the module's device, whichever is current
            with torch.cuda.device(plan.device):
                return plan(pilots, scores=scores)
        return plan(pilots, scores=scores)

    def forward(self, pilot_symbols: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return tuple(self.classify(pilot_symbols)[1:4])

    def get_model_info(self) -> dict:
        return {"model_name": self.__class__.__name__, "pilot_size": self.pilot_size, "assume": dict(self.assume), "window": self.window,
                "horizon": self.horizon, "pool": self.pool, "device": str(self.table_image.device), "total_parameters": 0,
                "trainable_parameters": 0}


class EstimatedConditions(nn.Module):
    """Any estimator with the reference's ``forward(pilot_symbols, meta_data)`` signature (``estimators.AdaFortiTranEstimator``,
    ``LmmseEstimator``), fed ESTIMATED conditions: the ``snr / ds / dop`` entries of the six-tuple ``(file_no, snr, ds, dop, n, types)``
    are replaced by ``ConditionEstimator(cfg, window, horizon, assume, pool)``'s, in the shape of the entries they replace (``[B, 1]``
    where ``meta_data`` is None, and the other four entries are then None); everything else passes through.  The estimated
    conditions stay on the chooser's device: on a HIP device nothing is read back.  ``evaluation.get_test_stats`` measures the wrapper
    like any estimator, which is how a blind AdaFortiTran is compared with a genie-aided one."""

    def __init__(self, model: nn.Module, cfg: ChannelSimConfig, window: int = 1, horizon: int = 0, assume=None, pool: bool = True) -> None:
        super().__init__()
        if not isinstance(model, nn.Module):
            raise ValueError(f"EstimatedConditions wraps an nn.Module with forward(pilot_symbols, meta_data); got {type(model).__name__}")
        self.model = model
        self.chooser = ConditionEstimator(cfg, window, horizon, assume, pool)

    def substitute(self, pilot_symbols: torch.Tensor, meta_data: Optional[tuple]) -> tuple:
        """The six-tuple the wrapped model sees."""
        est = self.chooser(pilot_symbols)
        if meta_data is None:
            return (None, *(c.reshape(-1, 1) for c in est), None, None)
        file_no, snr, ds, dop, n, types = meta_data
        shaped = [c.reshape(old.shape) if torch.is_tensor(old) and old.numel() == c.numel() else c.reshape(-1, 1)
                  for c, old in zip(est, (snr, ds, dop))]
        return (file_no, *shaped, n, types)

    def forward(self, pilot_symbols: torch.Tensor, meta_data: Optional[tuple] = None) -> torch.Tensor:
        return self.model(pilot_symbols, self.substitute(pilot_symbols, meta_data))

    def get_model_info(self) -> dict:
        inner = self.model.get_model_info() if hasattr(self.model, "get_model_info") else {"model_name": type(self.model).__name__}
        return {**inner, "model_name": f"EstimatedConditions({inner.get('model_name')})", "conditions": self.chooser.get_model_info()}
