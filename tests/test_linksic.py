"""``linksim``'s successive-cancellation link on the CPU: ``link_sic_host`` against a definition rebuilt from the documented streams
with NumPy's own linear algebra (the textbook MMSE filter, its SINR order, the subtraction of ``E[:, f] x^`` and maximum-ratio combining
of the residual), the order identity, the first-detected stream against ``link_sm_host`` exactly, the genie bound against the diversity
link, an unheard second stream, a tie, the refusals, the accumulators and sweeps with ``detector="sic"`` against the twin applied batch
by batch, ``sic_propagation``, the binding, the physical orderings, and the shares of dependent and flagged decisions on the inputs
tests/test_linksic_gpu.py compares the kernel on.

``derived_tau_sic`` / ``derived_e_lambda_sic`` are the bounds the GPU file derives in its docstring; it imports them, so both files speak
about the same arrays (``test_linksm.sm_inputs``) and the same bounds."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, linksim
from adafortitran_amd.chansim import SynthLoader, frame_keys, ls_interpolate, words
from adafortitran_amd.linksim import (ALL_DETECTORS, BITS_PER_SYMBOL, DETECTORS, BlockErrorAccumulator, CodeConfig, HarqAccumulator,
                                      LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator, constellation,
                                      detector_reg, link_decode_host, link_joint_host, link_ldpc_host, link_mrc_host, link_sm_host,
                                      noise_sigma, sm_weights)
from test_linkmrc import MRC_ODD
from test_linksim import GRIDS, TAU_CAP
from test_linksm import SM_SHARE_CAP, U, _brute_force, _detected, _e_m, _operands, _rebuilt, derived_e_lambda, derived_tau, sm_cases

DEPENDENT_CAP = 2e-2                                         # of the data elements, at the derived tau_sic(R)


# ---- the bounds of the float32 kernel (derived in the docstring of tests/test_linksic_gpu.py) ----

def _e_second(R: int):
    """(e_c2, e_g): the error of the second stage's ``c_o`` in units of ``reach(m_o) + G01 |x^|`` and of ``p_o = g_oo`` in units of itself."""
    e_x = (1 + U) ** 2 - 1
    e_g = (1 + U) ** (2 + R) - 1
    e_c2 = (1 + max(_e_m(R), (1 + e_g) * (1 + e_x) - 1)) * (1 + U) ** 2 - 1
    return float(e_c2), float(e_g)


def derived_tau_sic(R: int) -> float:
    e_c2, e_g = _e_second(R)
    return max(derived_tau(R), e_c2, float((1 + e_g) * (1 + U) ** 3 - 1))


def derived_e_lambda_sic(R: int) -> float:
    e_c2, e_g = _e_second(R)
    e_a = (1 + U) ** 2 - 1
    e_i = max((1 + e_a) * (1 + e_g), 1 + e_c2) * (1 + U) - 1
    e_mu = (1 + e_a) * (1 + U) * (1 + e_i) - 1
    e_d = 2 * e_mu + 2 * U * (1 + e_mu)
    return max(derived_e_lambda(R), float(e_d + U * (2 + e_d)))


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    for R in (2, 3, 4, 8):
        print(f"R = {R}: tau_sic = {derived_tau_sic(R) / U:.1f} u (second stage c_o {_e_second(R)[0] / U:.1f} u), "
              f"e_lambda_sic = {derived_e_lambda_sic(R) / U:.1f} u")
    assert derived_tau_sic(2) < derived_tau_sic(8) <= TAU_CAP and derived_e_lambda_sic(2) < derived_e_lambda_sic(8) <= TAU_CAP
    assert derived_tau_sic(8) >= derived_tau(8) and derived_e_lambda_sic(8) >= derived_e_lambda(8)


# ---- the definition rebuilt from the documented streams, with NumPy's own linear algebra ----

def _sent_words(cfg, keys, R):
    (S, T), m = cfg.sim.ofdm, cfg.bits_per_symbol
    q = np.arange(S * T, dtype=np.uint64).reshape(1, 1, S, T)
    return (words(keys.reshape(-1, R, 2)[:, 0, :, None, None], 5, q) >> np.uint64(64 - m)).astype(np.int64)      # [G, 2, S, T]


def _nearest(cfg, xhat):
    """The word whose symbol is nearest to ``xhat``, and that symbol."""
    pts = constellation(cfg.bits_per_symbol)
    w = np.abs(xhat[..., None] - pts).argmin(axis=-1)
    return w, pts[w]


def _textbook_sic(cfg, keys, ideal, est, sigma, rho, scale, R):
    """Ordered MMSE-SIC as a textbook writes it, per element: the MMSE filter and its SINRs by ``np.linalg`` (``test_linksm._detected``),
    the stream with the larger SINR decided to the nearest symbol, ``E[:, f] x^`` taken out of ``y``, the residual combined by
    maximum-ratio combining onto ``E[:, o]``.  Returns (f [G,S,T], sinr [G,2,S,T], wrong bits [G,2,S,T], llr [G,2,S,T,m])."""
    (S, T), m = cfg.sim.ofdm, cfg.bits_per_symbol
    G = len(keys) // (2 * R)
    x, y = _rebuilt(cfg, keys, ideal, sigma, R)
    w = rho.astype(np.float64).reshape(G, R, 2)[:, :, 0]
    sc = scale.astype(np.float64)
    xlin, sinr = _detected(cfg, y, est, w, 1.0 / sc, R)                          # MMSE: reg = 1 / scale, the scales powers of two
    f = sinr[:, 1] > sinr[:, 0]
    first = np.stack([~f, f], axis=1)
    E = est.astype(np.complex128).reshape(G, R, 2, S, T)
    x_f = np.where(f, xlin[:, 1], xlin[:, 0])
    _, decided = _nearest(cfg, x_f)
    E_f, E_o = np.where(f[:, None], E[:, :, 1], E[:, :, 0]), np.where(f[:, None], E[:, :, 0], E[:, :, 1])
    residual = y - E_f * decided[:, None]
    wr = w[:, :, None, None]
    c_o, p_o = (wr * E_o.conj() * residual).sum(axis=1), (wr * np.abs(E_o) ** 2).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        x_o = np.where(p_o > 0, c_o / np.where(p_o > 0, p_o, 1), 0)
    xhat = np.where(first, xlin, x_o[:, None])
    factor = np.where(first, sinr, (sc[:, None, None] * p_o)[:, None])
    decided_words, _ = _nearest(cfg, xhat)
    wrong = np.vectorize(lambda v: bin(v).count("1"))(decided_words ^ _sent_words(cfg, keys, R)) * cfg.data_mask
    return f, sinr, wrong, _brute_force(cfg, xhat, factor)


def _order(est, rho, R, ofdm):
    """f [G, S, T]: stream 1 is detected first, ``g11 > g00`` with the Gram diagonal summed as the definition sums it."""
    E = est.astype(np.complex128).reshape(-1, R, 2, *ofdm)
    w = rho.astype(np.float64).reshape(-1, R, 2)[:, :, 0, None, None]
    g = [sum(w[:, r] * (E[:, r, s].real ** 2 + E[:, r, s].imag ** 2) for r in range(R)) for s in (0, 1)]
    return g[1] > g[0]


def _pow2_scale(G):
    return (2.0 ** (np.arange(G) % 5 + 1)).astype(np.float32)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_twin_is_textbook_ordered_mmse_sic(m):
    """Decisions and LLRs of both streams against the textbook receiver on every data element whose SINRs are not within rounding of each
    other and whose decisions are not on a boundary (|Delta| of the nearest bit above 1e-9 q): wrong bits equal, LLRs to 1e-9 q."""
    for name, R, n in sm_cases():
        if name == "default_120x14" and R != 2:
            continue
        sim, n, keys, sigma, ideal, est, rho, _, _ = _operands(name, R)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        scale = _pow2_scale(G)
        reg = detector_reg(scale, "mmse")
        assert (reg.astype(np.float64) * scale == 1).all()
        f, sinr, wrong, llr = _textbook_sic(cfg, keys, ideal, est, sigma, rho, scale, R)
        got = linksim.link_sic_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, tau=1e-9, e_lambda=1e-9)
        order = got[6] == 2
        clear = np.abs(sinr[:, 1] - sinr[:, 0]) > 1e-9 * (sinr[:, 1] + sinr[:, 0])
        assert not (order & cfg.data_mask & clear).any()
        mask = cfg.data_mask & clear & (got[6] == 0)
        assert mask.sum() >= 0.99 * cfg.data_mask.sum() * G, (name, R)
        q = got[9]
        assert (np.abs(got[2] - llr) <= 1e-9 * q)[:, 0][mask].all() and (np.abs(got[2] - llr) <= 1e-9 * q)[:, 1][mask].all(), (name, R)
        settled = mask[:, None] & ~got[5].any(axis=-1)
        assert (got[4] == wrong)[settled].all(), (name, R)
        assert got[3][:, 0].tolist() == (f & cfg.data_mask).sum(axis=(1, 2)).tolist() or not clear.all()


def test_the_order_is_the_order_of_the_post_detection_sinrs():
    """``g11 > g00`` equals ``SINR_1 > SINR_0`` of the MMSE and of the ZF detector wherever the SINRs are not within 1e-9 of each other."""
    ties = 0
    for name, R, n in sm_cases():
        for which in ("lmmse", "ideal"):
            sim, n, keys, sigma, ideal, est, rho, _, _ = _operands(name, R, which)
            cfg, G = LinkConfig(sim, 2), n // (2 * R)
            S, T = sim.ofdm
            scale = _pow2_scale(G)
            _, y = _rebuilt(cfg, keys, ideal, sigma, R)
            w = rho.astype(np.float64).reshape(G, R, 2)[:, :, 0]
            E = est.astype(np.complex128).reshape(G, R, 2, S, T)
            g = (w[:, :, None, None, None] * np.abs(E) ** 2).sum(axis=1)         # [G, 2, S, T]
            for reg in (1.0 / scale.astype(np.float64), np.zeros(G)):
                _, sinr = _detected(cfg, y, est, w, reg, R)
                clear = np.abs(sinr[:, 1] - sinr[:, 0]) > 1e-9 * (sinr[:, 1] + sinr[:, 0])
                ties += int((~clear).sum())
                assert ((g[:, 1] > g[:, 0]) == (sinr[:, 1] > sinr[:, 0]))[clear].all(), (name, R, which)
    print(f"elements whose two SINRs are within 1e-9 of each other: {ties}")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_first_detected_stream_is_the_linear_detectors_exactly(m):
    for name, R, n in sm_cases():
        for which, detector in (("lmmse", "mmse"), ("ideal", "zf")):
            sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands(name, R, which, detector)
            cfg = LinkConfig(sim, m)
            sic = linksim.link_sic_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, tau=TAU_CAP)
            sm = link_sm_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, tau=TAU_CAP)
            f = _order(est, rho, R, sim.ofdm)
            first = np.stack([~f, f], axis=1)
            assert np.array_equal(sic[2][first], sm[2][first]) and np.array_equal(sic[4][first], sm[3][first])
            assert np.array_equal(sic[5][first], sm[4][first])
            assert sic[3][:, 0].tolist() == (f & cfg.data_mask).sum(axis=(1, 2)).tolist()
            wf, wo = np.where(f, sic[4][:, 1], sic[4][:, 0]), np.where(f, sic[4][:, 0], sic[4][:, 1])
            assert sic[3][:, 1].tolist() == (wf > 0).sum(axis=(1, 2)).tolist()
            assert sic[3][:, 2].tolist() == ((wf > 0) & (wo > 0)).sum(axis=(1, 2)).tolist()
            assert np.array_equal(sic[0][..., 0], sic[4].sum(axis=(2, 3))) and np.array_equal(sic[0][..., 1], (sic[4] > 0).sum(axis=(2, 3)))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_genie_with_the_channel_itself_is_the_diversity_link(m):
    """``genie=True`` and ``est = ideal``: the second stream's ``(c, p)`` are the diversity link's on the frames ``(r, o)`` with the noise
    of the frames ``(r, 0)`` -- seen through its decisions and LLRs, to 1e-9 q."""
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, _, rho, scale, reg = _operands(name, R, "ideal")
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        S, T = sim.ofdm
        got = linksim.link_sic_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, R, tau=1e-9, e_lambda=1e-9, genie=True)
        H = ideal.astype(np.complex128).reshape(G, R, 2, S, T)
        k = keys.reshape(G, R, 2)
        sg, w = sigma.astype(np.float64).reshape(G, R, 2), rho.astype(np.float64).reshape(G, R, 2)
        for o in (0, 1):
            gi, gq, x = linksim._sent(cfg, np.ascontiguousarray(k[:, 0, o]))
            c = p = reach = 0.0
            for r in range(R):
                noise = linksim._noise(cfg, np.ascontiguousarray(k[:, r, 0]), sg[:, r, 0])
                h = H[:, r, o]
                wr = w[:, r, 0, None, None]
                c, p = c + wr * ((h * x + noise) * h.conj()), p + wr * np.abs(h) ** 2
                reach = reach + wr * (np.abs(h) * np.abs(x) + np.abs(noise)) * np.abs(h)
            _, wrong, flags = linksim._hard(cfg, gi, gq, c, p, reach, 1e-9)
            _, llr, _, _, q = linksim._soft(cfg, gi, gq, c, p, reach, scale, (1.0,), 1e-9)
            f = _order(ideal, rho, R, sim.ofdm)
            second = (f if o == 0 else ~f) & cfg.data_mask                       # stream o is the second one
            assert second.any() or name == MRC_ODD
            assert (np.abs(got[2][:, o] - llr) <= 1e-9 * np.maximum(q, got[9][:, o]))[second].all(), (name, R, o)
            settled = second & ~flags.any(axis=-1)
            assert (got[4][:, o] == wrong)[settled].all(), (name, R, o)


def _unheard(name, R):
    sim, n, keys, sigma, ideal, est, rho, _, _ = _operands(name, R)
    H, E = ideal.copy(), est.copy()
    H[1::2], E[1::2] = 0, 0
    return sim, n, keys, sigma, ideal, est, H, E, rho


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_stream(m):
    """``H_r1 = E_r1 = 0``, ``scale = 2^k`` and ``reg = 2^-k``: stream 0 is the diversity link on the frames (r, 0), stream 1's LLRs are 0
    and no element is detected in swapped order."""
    for name, R, _ in sm_cases():
        sim, n, keys, sigma, ideal, est, H, E, rho = _unheard(name, R)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        scale = (2.0 ** (np.arange(G) % 4 + 1)).astype(np.float32)
        reg = (1.0 / scale).astype(np.float32)
        counts, loss, llr, stats = linksim.link_sic_host(cfg, keys, H, E, sigma, rho, scale, reg, R, 2, (1.0, 0.5))
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R, (1.0, 0.5), e_lambda=TAU_CAP)
        assert np.array_equal(counts[:, 0], want[0]) and (np.abs(llr[:, 0] - want[2]) <= 1e-12 * want[5]).all(), (name, R)
        np.testing.assert_allclose(loss[:, 0], want[1], rtol=1e-9, atol=0)
        assert not llr[:, 1].any() and np.allclose(loss[:, 1], m * cfg.data_elements) and not stats[:, 0].any()


def test_a_tie_detects_stream_0_first_everywhere():
    """``E_r1 = conj(E_r0)``: ``g00 == g11``, so ``f = 0`` on every element, and stream 0 is the linear detector's."""
    for name, R, _ in sm_cases():
        sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands(name, R)
        E = est.copy()
        E[1::2] = E[0::2].conj()
        cfg = LinkConfig(sim, 4)
        sic = linksim.link_sic_host(cfg, keys, ideal, E, sigma, rho, scale, reg, R)
        sm = link_sm_host(cfg, keys, ideal, E, sigma, rho, scale, reg, R)
        assert not sic[3][:, 0].any() and np.array_equal(sic[2][:, 0], sm[2][:, 0]) and np.array_equal(sic[0][:, 0], sm[0][:, 0])


def test_refusals_and_names():
    sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands("odd_30x7", 4)
    cfg = LinkConfig(sim, 4)
    assert linksim.SIC_DETECTOR == "sic" and DETECTORS == ("zf", "mmse") and ALL_DETECTORS == ("zf", "mmse", "joint")
    assert linksim.LINK2_DETECTORS == ("zf", "mmse", "joint", "sic")
    for bad in (1, 3, 0, 2.0, True, "2"):
        with pytest.raises(ValueError, match="streams"):
            linksim.link_sic_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, 4, bad)
    for bad in (0, 9, 2.0, -1, True, "2"):
        with pytest.raises(ValueError, match="branches"):
            linksim.link_sic_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, bad)
    with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
        linksim.link_sic_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, 1)
    with pytest.raises(ValueError, match="32 frames is not a multiple of branches \\* streams = 3 \\* 2"):
        linksim.link_sic_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, 3)
    for args, word in (((rho[:8], scale, reg), "rho"), ((rho, scale[:3], reg), "scale"), ((rho, scale, reg[:3]), "reg")):
        with pytest.raises(ValueError, match=word):
            linksim.link_sic_host(cfg, keys, ideal, ideal, sigma, *args, 4)
    with pytest.raises(ValueError, match="between 1 and 8 factors"):
        linksim.link_sic_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, 4, 2, np.ones(9))
    for bad in ("sic", "ml"):                                                    # the regulariser stays the linear detectors'
        with pytest.raises(ValueError, match="detector"):
            detector_reg(scale, bad)
        with pytest.raises(ValueError, match="detector"):
            sm_weights(np.zeros(8), 0.0, 2, 2, bad)
    for bad in ("ml", "SIC", "vblast", None):
        with pytest.raises(ValueError, match="detector"):
            LinkAccumulator(cfg, "cpu", branches=2, streams=2, detector=bad)
    with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
        LinkAccumulator(cfg, "cpu", streams=2, detector="sic")
    with pytest.raises(ValueError, match="6 frames is not a multiple of branches \\* streams = 2 \\* 2"):
        LinkAccumulator(cfg, "cpu", branches=2, streams=2, detector="sic").update(
            None, torch.from_numpy(ideal[:6].copy()), frame_ids=np.arange(6), snr_db=np.zeros(6))
    one = LinkAccumulator(cfg, "cpu", detector="sic")                            # one stream ignores the detector
    for acc in (one, LinkAccumulator(cfg, "cpu", branches=2, streams=2), LinkAccumulator(cfg, "cpu", branches=2, streams=2, detector="joint")):
        with pytest.raises(ValueError, match="sic_propagation needs"):
            acc.sic_propagation()
    assert "streams" not in inspect.signature(HarqAccumulator.__init__).parameters
    assert "detector" not in inspect.signature(HarqAccumulator.__init__).parameters


class _Ls(torch.nn.Module):
    def __init__(self, sim):
        super().__init__()
        self.sim = sim
        self.register_buffer("anchor", torch.zeros(1))

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.cpu().numpy()))


def test_accumulators_sweeps_and_propagation_with_sic_on_the_host():
    """Each accumulator and each sweep equals ``link_sic_host`` (MMSE regulariser) applied batch by batch, the coded ones through the host
    decoders on its LLRs rounded to float32 with the keys of frames (0, s); ``sic_propagation`` is the twin's three sums as shares."""
    from adafortitran_amd.evaluation import get_link_bler, get_link_rates, get_link_stats
    R, N, seed, err_var = 2, 2, 5, 0.01
    sim = GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code, ldpc = CodeConfig(cfg, 64, "1/2"), LdpcConfig(cfg, (3, 6))
    factors = (1.0, 0.5)
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 8, 24, device="cpu", seed=seed))
    kw = dict(branches=R, streams=N, detector="sic")
    hard, rate = LinkAccumulator(cfg, "cpu", seed, **kw), RateAccumulator(cfg, "cpu", seed, factors, err_var, **kw)
    conv, lay = BlockErrorAccumulator(code, "cpu", seed, err_var, **kw), LdpcBlockErrorAccumulator(ldpc, "cpu", seed, err_var, R, N, "sic")
    mmse = LinkAccumulator(cfg, "cpu", seed, branches=R, streams=N)
    want = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "loss0": np.zeros(8), "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64),
            "conv0": np.zeros(2, np.int64), "stats": np.zeros(3, np.int64)}
    for pilots, ideal, meta in batches:
        est = model(pilots)
        for acc in (hard, rate, conv, lay, mmse):
            acc.update(est, ideal, meta)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        sent_keys = np.ascontiguousarray(keys.reshape(-1, R, N)[:, 0, :]).reshape(-1)
        snr = meta[1].numpy().reshape(-1)
        for ev, tag in ((0.0, "0"), (err_var, "")):
            rho, scale, reg = sm_weights(snr, ev, R, N, "mmse")
            *out, stats = linksim.link_sic_host(cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), rho, scale, reg, R, N,
                                                factors if tag == "" else np.asarray([2.0 ** -k for k in range(8)]))
            counts, loss, llr = (v.reshape(-1, *v.shape[2:]) for v in out)
            if tag == "0":
                want["hard"] += counts.sum(axis=0)
                want["stats"] += stats.sum(axis=0)
                want["loss0"] += loss.sum(axis=0)
                want["conv0"] += link_decode_host(code, sent_keys, llr.astype(np.float32))[0].sum(axis=0)
            else:
                want["loss"] += loss.sum(axis=0)
                want["conv"] += link_decode_host(code, sent_keys, llr.astype(np.float32))[0].sum(axis=0)
                want["ldpc"] += link_ldpc_host(ldpc, sent_keys, llr.astype(np.float32))[0].sum(axis=0)
    F = 12                                                                       # frames counts G N: per stream
    assert hard.frames == rate.frames == conv.frames == lay.frames == F and hard.detector == "sic"
    assert hard.errors.tolist() == want["hard"].tolist() and hard.result() == want["hard"][0] / (F * cfg.bits_per_frame)
    assert hard.result_ser() == want["hard"][1] / (F * cfg.data_elements)
    assert np.array_equal(rate.loss.numpy(), want["loss"])
    assert rate.result() == [4 - v / (F * cfg.data_elements) for v in want["loss"]]
    assert conv.errors.tolist() == want["conv"].tolist() and conv.result() == want["conv"][1] / (F * code.blocks)
    assert lay.errors.tolist() == want["ldpc"].tolist() and lay.result() == want["ldpc"][1] / (F * ldpc.blocks)
    assert 0 < want["hard"][0] < F * cfg.bits_per_frame // 2 and hard.errors.tolist() != mmse.errors.tolist()
    swapped, wrong, both = (int(v) for v in want["stats"])
    elements = F // N * cfg.data_elements
    assert 0 < both <= wrong < elements and 0 < swapped < elements
    assert hard.sic_propagation() == (swapped / elements, wrong / elements, both / wrong)
    loaders = [("SNR_0", SynthLoader(sim, 8, 24, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_stats(model, loaders, cfg, seed, **kw) == {0: want["hard"][0] / (F * cfg.bits_per_frame)}
    assert get_link_rates(model, loaders, cfg, seed, **kw) == {0: max(4 - v / (F * cfg.data_elements) for v in want["loss0"])}
    assert get_link_bler(model, loaders, code, seed, **kw) == {0: want["conv0"][1] / (F * code.blocks)}
    assert get_link_bler(model, loaders, ldpc, seed, err_var, **kw) == {0: want["ldpc"][1] / (F * ldpc.blocks)}


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    assert _abi.AFT_ABI_VERSION == 10
    restype, argtypes = _abi.SIGNATURES["aft_link_sic_f32"]
    sm = _abi.SIGNATURES["aft_link_sm_f32"][1]
    assert "aft_link_sic_f32" in _abi.EXPORTED_SYMBOLS and restype is C.c_int and len(argtypes) == 18
    assert argtypes == sm[:15] + [C.c_void_p] + sm[15:]                          # aft_link_sm_f32's list with stats behind llr
    assert argtypes[0]._type_ is _abi.AftLink and [i for i, t in enumerate(argtypes) if t is C.c_int] == [9, 10, 11, 16]
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "adafortitran_amd.h")).read()
    declared = re.findall(r"^(?:int|size_t|const char \*)\s*(aft_\w+)\(", header, flags=re.M)
    names = list(_abi.SIGNATURES)
    assert declared.count("aft_link_sic_f32") == 1 and declared.index("aft_link_sic_f32") == names.index("aft_link_sic_f32")


def _pooled_ber(cfg, counts):
    return float(counts[..., 0].sum()) / (counts.shape[0] * counts.shape[1] * cfg.bits_per_frame)


def test_physical_orderings():
    """On ``default_120x14`` with the channel itself: pooled BER joint <= sic <= mmse for m = 2 at R in (3, 4) and m = 4 at R in (2, 3, 4),
    and the first-detected stream's BER is below the second's."""
    for m, Rs in ((2, (3, 4)), (4, (2, 3, 4))):
        for R in Rs:
            sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands("default_120x14", R, "ideal")
            cfg = LinkConfig(sim, m)
            sic = linksim.link_sic_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, tau=0.0)
            mmse = link_sm_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R)
            joint = link_joint_host(cfg, keys, ideal, est, sigma, rho, scale, R)
            genie = linksim.link_sic_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, genie=True)
            ber = [_pooled_ber(cfg, v[0]) for v in (joint, sic, mmse)]
            swapped = sic[3][:, 0].sum()
            elements = cfg.data_elements * len(sic[0])
            f = _order(est, rho, R, sim.ofdm)
            first = np.where(f, sic[4][:, 1], sic[4][:, 0]).sum() / (elements * m)
            second = np.where(f, sic[4][:, 0], sic[4][:, 1]).sum() / (elements * m)
            print(f"m = {m}, R = {R}: BER joint {ber[0]:.4f} sic {ber[1]:.4f} mmse {ber[2]:.4f} genie {_pooled_ber(cfg, genie[0]):.4f}; "
                  f"first-detected {first:.4f}, second {second:.4f}; swapped {swapped / elements:.3f}")
            assert ber[0] <= ber[1] <= ber[2], (m, R, ber)
            assert first < second, (m, R, first, second)
            assert _pooled_ber(cfg, genie[0]) <= ber[1]


# ---- the dependent and flagged shares on the inputs the GPU tests use ----

def sic_shares(cfg, out, f):
    """(dependent elements as a share of the data elements, the second stream's own flagged (element, axis) pairs as a share of the
    data (element, axis) pairs, order-flagged elements as a share of the data elements) of ``link_sic_host(..., tau=...)``'s tuple
    ``out`` with the order ``f``."""
    flags, dep = out[5], out[6]
    elements = cfg.data_elements * len(dep)
    if not elements:
        return 0.0, 0.0, 0.0
    second = np.stack([f, ~f], axis=1)                                           # [G, N, S, T]: stream s is the second-detected one
    return float((dep > 0).sum()) / elements, float(flags[second].sum()) / (2 * elements), float((dep == 2).sum()) / elements


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_dependent_and_flagged_shares_on_the_inputs_the_gpu_tests_use(m):
    """At the derived tau_sic(R): dependent elements at most 2e-2 of the data elements, the second stream's own flagged (element, axis)
    pairs at most ``SM_SHARE_CAP``; the observed maxima, the order-flagged share among them, are printed."""
    worst = [(-1.0, ())] * 3
    for name, R, _ in sm_cases():
        for which in ("lmmse", "ideal"):
            sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands(name, R, which)
            cfg = LinkConfig(sim, m)
            out = linksim.link_sic_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, tau=derived_tau_sic(R))
            shares = sic_shares(cfg, out, _order(est, rho, R, sim.ofdm))
            assert shares[0] <= DEPENDENT_CAP and shares[1] <= SM_SHARE_CAP, (name, R, which, shares)
            worst = [max(w, (s, (name, R, which))) for w, s in zip(worst, shares)]
    print(f"m = {m}: largest shares at tau_sic(R): dependent {worst[0][0]:.2e} at {worst[0][1]}, flagged {worst[1][0]:.2e} at {worst[1][1]}, "
          f"order-flagged {worst[2][0]:.2e}")
