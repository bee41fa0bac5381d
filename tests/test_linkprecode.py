"""``linksim``'s closed-loop link on the CPU: ``precoding_subbands`` on every grid, ``link_precoded_host`` and ``precoding_pmi_host``
against a brute force rebuilt element by element from the documented streams (the PMI from the four sums ``sum rho |E_r0 + q_i
E_r1|^2``, the LLRs from ``scale |c - p a|^2 / p`` over all ``2^m`` symbols), the exact extremes, an unheard second antenna against the
diversity link, a turn of the second antenna by ``j``, a forced ``pmi=``, the refusals, the four accumulators and the three sweeps of
``evaluation`` with ``precoding_subband=`` against the definition applied batch by batch, the binding, the conditions on the inputs
tests/test_linkprecode_gpu.py compares the kernel on -- PMI-flagged subbands at ``PMI_TAU_CAP`` and flagged decisions at ``TAU_CAP``,
asserted here on the twin alone --, and the compiler's register report of the kernel.

The inputs are tests/test_linkalamouti.py's ``al_inputs`` / ``al_cases`` (seed 3): ``straddle_9x6`` and ``odd_last_alone_3x5`` are the
small grids, ``odd_30x7`` and ``default_120x14`` the large ones.  ``SUBBANDS`` are B = 1 (one PMI per subcarrier), 4, 7 (short last
subbands of 1 of 9 and 2 of 30 subcarriers) and S (one wideband PMI), and 60 on the default grid, whose two subbands the kernel sums
with two waves each; a B beyond a grid's S is left out there."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi
from adafortitran_amd.chansim import SynthLoader, frame_keys, words
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, CODEBOOK, MAX_SUBBANDS, BlockErrorAccumulator, CodeConfig, HarqAccumulator,
                                      LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator,
                                      alamouti_weights, constellation, link_decode_host, link_ldpc_host, link_mrc_host,
                                      link_precoded_host, noise_sigma, precoding_pmi_host, precoding_subbands, precoding_weights)
from test_linkalamouti import AL_GRIDS, LARGE, SMALL, STRADDLE, _Ls, _constant_channels, al_cases, al_inputs, al_operands
from test_linkmrc import MRC_ODD
from test_linksim import GRIDS, SHARE_CAP, TAU_CAP, flagged_share

PMI_TAU_CAP = 1e-4                                              # the issue's: at most one PMI-flagged subband per case there
SUBBANDS = (1, 4, 7, 60, None)                                  # None: B = S, one wideband PMI; 60: two halves of the default grid
ROTATED = np.array([3, 2, 0, 1])                                # where a turn of the second antenna by j sends each index


def widths(name):
    """The subband widths of a grid: ``SUBBANDS`` with None as S, those that fit, each once."""
    S = al_inputs(name)[0].ofdm[0]
    return sorted({S if B is None else B for B in SUBBANDS if B is None or B <= S})


def pc_cases():
    """(grid, R, frames used, B): ``al_cases`` times the grid's subband widths."""
    return [(name, R, n, B) for name, R, n in al_cases() for B in widths(name)]


# ---- the subbands ----

def test_the_subband_map_on_every_grid():
    assert [widths(name) for name in (STRADDLE, MRC_ODD, "odd_30x7", "default_120x14")] == [[1, 4, 7, 9], [1, 3], [1, 4, 7, 30],
                                                                                          [1, 4, 7, 60, 120]]
    for name in AL_GRIDS:
        cfg = LinkConfig(al_inputs(name)[0], 4)
        S = cfg.sim.ofdm[0]
        for B in range(1, S + 1):
            index, n_sub = precoding_subbands(cfg, B)
            assert index.dtype == np.int64 and index.shape == (S,) and n_sub == -(-S // B) == index[-1] + 1
            sizes = np.bincount(index)
            assert (sizes[:-1] == B).all() and sizes[-1] == S - (n_sub - 1) * B and 1 <= sizes[-1] <= B and (np.diff(index) >= 0).all()
    cfg = LinkConfig(al_inputs(STRADDLE)[0], 4)
    assert precoding_subbands(cfg, 4)[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2] and precoding_subbands(cfg, 9) [1] == 1
    cfg = LinkConfig(al_inputs("odd_30x7")[0], 4)
    assert np.bincount(precoding_subbands(cfg, 7)[0]).tolist() == [7, 7, 7, 7, 2]
    assert MAX_SUBBANDS == _abi.AFT_LINK_MAX_SUBBANDS == 1024 and precoding_weights is alamouti_weights
    assert CODEBOOK == (1, -1, 1j, -1j)


# ---- the definition ----

def _rebuilt(cfg, keys, ideal, est, sigma, rho, R, B):
    """(x, c, p [G,S,T], pmi [G,n_sub]) as the module docstring writes them, subband by subband and element by element in plain loops
    from the documented streams: float64, independent of the twin's helpers.  The PMI is the first index whose
    ``sum rho |E_r0 + q_i E_r1|^2`` over the subband is the largest."""
    (S, T), m = cfg.sim.ofdm, cfg.bits_per_symbol
    W = 2 * R
    G = len(keys) // W
    q = np.arange(S * T, dtype=np.uint64).reshape(1, S, T)
    x = constellation(m)[(words(keys[::W, None, None], 5, q) >> np.uint64(64 - m)).astype(np.int64)]
    H = ideal.astype(np.complex128).reshape(G, R, 2, S, T)
    E = est.astype(np.complex128).reshape(G, R, 2, S, T)
    k0 = keys.reshape(G, R, 2)[:, :, 0]
    u1, u2 = (((words(k0[:, :, None, None], s, q[None]) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23 for s in (6, 7))
    noise = sigma.astype(np.float64).reshape(G, R, 2)[:, :, 0, None, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)
    w = rho.astype(np.float64).reshape(G, R, 2)[:, :, 0]
    n_sub = (S + B - 1) // B
    c, p, pmi = np.zeros((G, S, T), complex), np.zeros((G, S, T)), np.zeros((G, n_sub), np.int32)
    book = (1, -1, 1j, -1j)
    for b in range(n_sub):
        rows = range(b * B, min(S, (b + 1) * B))
        power = np.zeros((G, 4))
        for i, qi in enumerate(book):
            for s in rows:
                for t in range(T):
                    for r in range(R):
                        power[:, i] += w[:, r] * np.abs(E[:, r, 0, s, t] + qi * E[:, r, 1, s, t]) ** 2
        pmi[:, b] = power.argmax(axis=1)
        for g in range(G):
            qi = book[pmi[g, b]]
            for s in rows:
                for r in range(R):
                    y = H[g, r, 0, s] * x[g, s] + H[g, r, 1, s] * (qi * x[g, s]) + noise[g, r, s]
                    e = E[g, r, 0, s] + qi * E[g, r, 1, s]
                    c[g, s] += w[g, r] * (y * e.conj())
                    p[g, s] += w[g, r] * np.abs(e) ** 2
    return x, c, p, pmi


def _brute_force(cfg, c, p, scale):
    """[G,S,T,m]: min over the symbols with bit 1 minus min over those with bit 0 of ``scale |c - p a|^2 / p``."""
    m, pts = cfg.bits_per_symbol, constellation(cfg.bits_per_symbol)
    safe = np.where(p > 0, p, 1.0)
    dist = scale.astype(np.float64)[:, None, None, None] * np.abs(c[..., None] - p[..., None] * pts) ** 2 / safe[..., None]
    word = np.arange(1 << m)
    out = np.empty((*c.shape, m))
    for j in range(m):
        one = ((word >> (m - 1 - j)) & 1).astype(bool)
        out[..., j] = dist[..., one].min(axis=-1) - dist[..., ~one].min(axis=-1)
    return out * cfg.data_mask[None, :, :, None]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_pmi_and_llrs_against_a_brute_force(m):
    """Pins the subbands, the codebook and its order, the tie-free selection, the weights, the precoded sample, the effective estimate,
    the separable form, the bit order and the leader's scale: the PMI exactly (no subband of these inputs is near a tie), the LLRs
    to 1e-9 q."""
    seen = set()
    for name, R in ((STRADDLE, 1), (STRADDLE, 2), ("odd_30x7", 3), (MRC_ODD, 2)):
        sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R, "lmmse", 0.01)
        cfg = LinkConfig(sim, m)
        for B in widths(name):
            out = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, e_lambda=TAU_CAP)
            llr, q, pmi = out[2], out[5], out[-1]
            _, c, p, want_pmi = _rebuilt(cfg, keys, ideal, est, sigma, rho, R, B)
            assert len(out) == 7 and pmi.dtype == np.int32 and np.array_equal(pmi, want_pmi), (name, R, B)
            assert np.array_equal(pmi, precoding_pmi_host(cfg, est, rho, R, B))
            assert not precoding_pmi_host(cfg, est, rho, R, B, 1e-9)[1].any()
            want = _brute_force(cfg, c, p, scale)
            assert llr.shape == want.shape == q.shape == (n // (2 * R), *sim.ofdm, m)
            assert (np.abs(llr - want) <= 1e-9 * q).all(), (name, R, B, float((np.abs(llr - want) / np.where(q > 0, q, 1)).max()))
            assert (q[:, cfg.data_mask] > 0).all() and (q[:, ~cfg.data_mask] == 0).all()
            seen |= set(pmi.reshape(-1).tolist())
    assert seen == {0, 1, 2, 3}                                                  # every index occurs


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_exact_extremes(m):
    """One constant per frame as the channel, the estimates are the channels and there is no noise: no bit is wrong, nothing is
    flagged, and ``p >= sum rho (|H_r0|^2 + |H_r1|^2)`` at every data element -- the chosen precoder never loses to a single
    antenna."""
    for name, R, n, B in pc_cases():
        sim, n, keys, sigma, _, _, rho, scale = al_operands(name, R)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        H, zero = _constant_channels(n, *sim.ofdm), np.zeros_like(sigma)
        counts, loss, llr, wrong, flags, pmi = link_precoded_host(cfg, keys, H, H, zero, rho, scale, R, B, tau=TAU_CAP)
        assert counts.shape == (G, 2) and counts.dtype == np.int64 and loss.shape == (G, 1) and llr.shape == (G, *sim.ofdm, m)
        assert wrong.shape == (G, *sim.ofdm) and flags.shape == (G, *sim.ofdm, 2) and pmi.shape == (G, -(-sim.ofdm[0] // B))
        assert not counts.any() and not wrong.any() and not flags.any(), (name, R, B)
        assert not llr[:, ~cfg.data_mask].any() and (llr[:, cfg.data_mask] != 0).all()
        assert not precoding_pmi_host(cfg, H, rho, R, B, PMI_TAU_CAP)[1].any()
        # p of the chosen precoders, formed here from the definition's pmi, against both antennas' powers added without array gain
        Hc = H.astype(np.complex128)
        single = sum(rho[2 * r::2 * R, None, None].astype(np.float64) * (np.abs(Hc[2 * r::2 * R]) ** 2 + np.abs(Hc[2 * r + 1::2 * R]) ** 2)
                     for r in range(R))
        index = precoding_subbands(cfg, B)[0]
        e = [Hc[2 * r::2 * R] + np.asarray(CODEBOOK)[pmi[:, index]][:, :, None] * Hc[2 * r + 1::2 * R] for r in range(R)]
        p = sum(rho[2 * r::2 * R, None, None].astype(np.float64) * np.abs(e[r]) ** 2 for r in range(R))
        assert (p >= single * (1 - 1e-12)).all(), (name, R, B)
        assert (pmi == pmi[:, :1]).all()                                          # a constant channel: one precoder for the whole band


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_antenna_is_the_diversity_link(m):
    """``H_r1 = E_r1 = 0``: every ``g_b`` is 0 and every PMI 0; wrong bits and LLRs equal ``link_mrc_host`` on the frames (r, 0) at
    every data element, exactly."""
    for name, R, n, B in pc_cases():
        sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R)
        cfg = LinkConfig(sim, m)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        _, _, llr, wrong, _, pmi = link_precoded_host(cfg, keys, H, E, sigma, rho, scale, R, B, tau=TAU_CAP)
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R, tau=TAU_CAP)
        assert not pmi.any() and np.array_equal(wrong, want[3]) and np.array_equal(llr, want[2]), (name, R, B)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_turn_of_the_second_antenna_by_j(m):
    """``H_r1, E_r1 -> j H_r1, j E_r1``: LLRs, counts and losses exactly equal, the PMI mapped 0 -> 3, 1 -> 2, 2 -> 0, 3 -> 1 at
    unflagged subbands."""
    for name, R, n, B in pc_cases():
        sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R)
        cfg = LinkConfig(sim, m)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 1j * ideal[1::2], 1j * est[1::2]
        assert np.array_equal(H[1::2].real, -ideal[1::2].imag) and np.array_equal(H[1::2].imag, ideal[1::2].real)    # the turn is exact
        want = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, (1.0, 0.5))
        got = link_precoded_host(cfg, keys, H, E, sigma, rho, scale, R, B, (1.0, 0.5))
        clear = ~precoding_pmi_host(cfg, est, rho, R, B, PMI_TAU_CAP)[1]
        assert clear.any() and np.array_equal(got[3][clear], ROTATED[want[3]][clear]), (name, R, B)
        if clear.all():
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])), (name, R, B)


def test_a_forced_pmi_is_honoured():
    """``pmi=`` replaces the selection: the selected indices given back reproduce the outputs bit for bit, and the index opposite to
    the selected one (q -> -q) gives a smaller ``p`` -- read off the LLRs at m = 2, whose magnitudes it scales -- and more errors."""
    for name, R, B in ((STRADDLE, 2, 4), ("odd_30x7", 1, 7), ("odd_30x7", 4, 30), (MRC_ODD, 1, 1)):
        sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R, "ideal")
        cfg = LinkConfig(sim, 2)
        zero = np.zeros_like(sigma)
        best = link_precoded_host(cfg, keys, ideal, est, zero, rho, scale, R, B)
        again = link_precoded_host(cfg, keys, ideal, est, zero, rho, scale, R, B, pmi=best[3])
        assert all(np.array_equal(a, b) for a, b in zip(best, again))
        worst = link_precoded_host(cfg, keys, ideal, est, zero, rho, scale, R, B, pmi=best[3] ^ 1)
        assert np.array_equal(worst[3], best[3] ^ 1)
        # E = H and no noise: c = p x, so |llr| = 4 d scale p |x_axis| = 4 d^2 scale p on both axes
        pb, pw = np.abs(best[2][..., 0]).sum(axis=(1, 2)), np.abs(worst[2][..., 0]).sum(axis=(1, 2))       # per group
        assert (pw < pb).all(), (name, R, B, pw, pb)
        for bad in (best[3][:-1], best[3] + 4, best[3] - 4, best[3].astype(np.float64), best[3].reshape(-1)):
            with pytest.raises(ValueError, match="pmi"):
                link_precoded_host(cfg, keys, ideal, est, zero, rho, scale, R, B, pmi=bad)


def test_refusals():
    sim, n, keys, sigma, ideal, est, rho, scale = al_operands("odd_30x7", 4)
    cfg = LinkConfig(sim, 4)
    code = CodeConfig(cfg, 64)
    for bad in (0, 31, -1, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="precoding_subband"):
            link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, 4, bad)
        with pytest.raises(ValueError, match="precoding_subband"):
            precoding_subbands(cfg, bad)
        with pytest.raises(ValueError, match="precoding_subband"):
            precoding_pmi_host(cfg, est, rho, 4, bad)
        if bad is not None:
            for make in (lambda: LinkAccumulator(cfg, "cpu", precoding_subband=bad), lambda: RateAccumulator(cfg, "cpu", precoding_subband=bad),
                         lambda: BlockErrorAccumulator(code, "cpu", precoding_subband=bad),
                         lambda: LdpcBlockErrorAccumulator(LdpcConfig(cfg, (3, 6)), "cpu", precoding_subband=bad)):
                with pytest.raises(ValueError, match="precoding_subband"):
                    make()
    for bad in (0, 9, 2.0, -1, True, "2"):
        with pytest.raises(ValueError, match="branches"):
            link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, bad, 4)
        with pytest.raises(ValueError, match="branches"):
            precoding_pmi_host(cfg, est, rho, bad, 4)
        with pytest.raises(ValueError, match="branches"):
            LinkAccumulator(cfg, "cpu", branches=bad, precoding_subband=4)
    with pytest.raises(ValueError, match="32 frames is not a multiple of branches \\* 2 = 3 \\* 2"):
        link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, 3, 4)
    with pytest.raises(ValueError, match="32 frames is not a multiple of branches \\* 2 = 3 \\* 2"):
        precoding_pmi_host(cfg, est, rho, 3, 4)
    with pytest.raises(ValueError, match="rho"):
        link_precoded_host(cfg, keys, ideal, est, sigma, rho[:8], scale, 4, 4)
    with pytest.raises(ValueError, match="scale"):
        link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale[:3], 4, 4)
    ldpc = LdpcConfig(cfg, (3, 6))
    for make in (lambda **kw: LinkAccumulator(cfg, "cpu", branches=2, precoding_subband=4, **kw),
                 lambda **kw: RateAccumulator(cfg, "cpu", branches=2, precoding_subband=4, **kw),
                 lambda **kw: BlockErrorAccumulator(code, "cpu", branches=2, precoding_subband=4, **kw),
                 lambda **kw: LdpcBlockErrorAccumulator(ldpc, "cpu", branches=2, precoding_subband=4, **kw)):
        with pytest.raises(ValueError, match="precoding_subband.*streams must be 1"):
            make(streams=2)
        for pairing in ("time", "frequency"):
            with pytest.raises(ValueError, match="precoding_subband.*tx_diversity None"):
                make(tx_diversity=pairing)
        with pytest.raises(ValueError, match="6 frames is not a multiple of branches \\* 2 = 2 \\* 2"):
            make().update(None, torch.from_numpy(ideal[:6].copy()), frame_ids=np.arange(6), snr_db=np.zeros(6))
    LinkAccumulator(cfg, "cpu", detector="anything", precoding_subband=4)        # the detector is ignored
    with pytest.raises(ValueError, match="pmi_histogram needs precoding_subband"):
        LinkAccumulator(cfg, "cpu").pmi_histogram()
    # more than 1024 subbands
    from adafortitran_amd.chansim import ChannelSimConfig
    wide = LinkConfig(ChannelSimConfig(ofdm=(1025, 2), pilot=(5, 2)), 2)
    with pytest.raises(ValueError, match="1025 subbands of the 1025 subcarriers, more than 1024"):
        precoding_subbands(wide, 1)
    assert precoding_subbands(wide, 2)[1] == 513
    assert "precoding_subband" not in inspect.signature(HarqAccumulator.__init__).parameters
    for cls in (LinkAccumulator, RateAccumulator, BlockErrorAccumulator, LdpcBlockErrorAccumulator):
        par = inspect.signature(cls.__init__).parameters["precoding_subband"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("B", (7, 30))
def test_accumulators_and_sweeps_with_precoding_on_the_host(B):
    """A host ``SynthLoader`` (every frame at its own SNR), three batches of eight frames (two groups of 2 x 2): each accumulator and
    each sweep equals the definition applied batch by batch, the coded ones through the host decoders on the definition's LLRs rounded
    to float32 with the leaders' keys; the histogram counts the definition's PMIs."""
    from adafortitran_amd.evaluation import get_link_bler, get_link_rates, get_link_stats
    R, seed, err_var = 2, 5, 0.01
    sim = GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code, ldpc = CodeConfig(cfg, 64, "1/2"), LdpcConfig(cfg, (3, 6))
    factors = (1.0, 0.5)
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 8, 24, device="cpu", seed=seed))
    assert len(batches) == 3
    kw = dict(branches=R, precoding_subband=B)
    hard, rate = LinkAccumulator(cfg, "cpu", seed, **kw), RateAccumulator(cfg, "cpu", seed, factors, err_var, **kw)
    conv, lay = BlockErrorAccumulator(code, "cpu", seed, err_var, **kw), LdpcBlockErrorAccumulator(ldpc, "cpu", seed, err_var, **kw)
    want = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "loss0": np.zeros(8), "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64),
            "conv0": np.zeros(2, np.int64), "pmi": np.zeros(4, np.int64)}
    for pilots, ideal, meta in batches:
        est = model(pilots)
        for acc in (hard, rate, conv, lay):
            acc.update(est, ideal, meta)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        lead = np.ascontiguousarray(keys[::2 * R])
        snr = meta[1].numpy().reshape(-1)
        for ev, tag in ((0.0, "0"), (err_var, "")):
            rho, scale = precoding_weights(snr, ev, R)
            counts, loss, llr, pmi = link_precoded_host(cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), rho, scale, R, B,
                                                        factors if tag == "" else np.asarray([2.0 ** -k for k in range(8)]))
            if tag == "0":
                want["hard"] += counts.sum(axis=0)
                want["loss0"] += loss.sum(axis=0)
                want["conv0"] += link_decode_host(code, lead, llr.astype(np.float32))[0].sum(axis=0)
                want["pmi"] += np.bincount(pmi.reshape(-1), minlength=4)
            else:
                want["loss"] += loss.sum(axis=0)
                want["conv"] += link_decode_host(code, lead, llr.astype(np.float32))[0].sum(axis=0)
                want["ldpc"] += link_ldpc_host(ldpc, lead, llr.astype(np.float32))[0].sum(axis=0)
    F = 6                                                                        # frames counts the groups
    assert hard.frames == rate.frames == conv.frames == lay.frames == F and hard.precoding_subband == B and hard.tx_diversity is None
    assert hard.errors.tolist() == want["hard"].tolist() and hard.result() == want["hard"][0] / (F * cfg.bits_per_frame)
    assert hard.result_ser() == want["hard"][1] / (F * cfg.data_elements)
    assert np.array_equal(rate.loss.numpy(), want["loss"])
    assert rate.result() == [4 - v / (F * cfg.data_elements) for v in want["loss"]]
    assert conv.errors.tolist() == want["conv"].tolist() and conv.result() == want["conv"][1] / (F * code.blocks)
    assert lay.errors.tolist() == want["ldpc"].tolist() and lay.result() == want["ldpc"][1] / (F * ldpc.blocks)
    assert 0 < want["hard"][0] < F * cfg.bits_per_frame // 2                       # the frames are not trivial
    for acc in (hard, rate, conv, lay):                                          # the PMIs do not depend on err_var: rho is a ratio ...
        got = acc.pmi_histogram()
        assert sum(got) == F * -(-30 // B) and all(isinstance(v, int) for v in got)
    assert hard.pmi_histogram() == want["pmi"].tolist()                          # ... to rounding; the hard one has err_var = 0
    loaders = [("SNR_0", SynthLoader(sim, 8, 24, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_stats(model, loaders, cfg, seed, **kw) == {0: want["hard"][0] / (F * cfg.bits_per_frame)}
    assert get_link_rates(model, loaders, cfg, seed, **kw) == {0: max(4 - v / (F * cfg.data_elements) for v in want["loss0"])}
    assert get_link_bler(model, loaders, code, seed, **kw) == {0: want["conv0"][1] / (F * code.blocks)}
    assert get_link_bler(model, loaders, ldpc, seed, err_var, **kw) == {0: want["ldpc"][1] / (F * ldpc.blocks)}
    with pytest.raises(ValueError, match="streams must be 1"):
        get_link_stats(model, loaders, cfg, seed, branches=R, streams=2, precoding_subband=B)
    with pytest.raises(ValueError, match="tx_diversity None"):
        get_link_rates(model, loaders, cfg, seed, branches=R, tx_diversity="time", precoding_subband=B)


def test_without_precoding_the_objects_are_todays():
    """``precoding_subband=None``: the same outputs as a call without the keyword, ``np.array_equal``, on every accumulator and for
    every other mode."""
    seed, sim = 5, GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code = CodeConfig(cfg, 64, "1/2")
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 8, 16, device="cpu", seed=seed))
    for kw in (dict(branches=1), dict(branches=2), dict(branches=2, streams=2), dict(branches=2, tx_diversity="time")):
        for make, read in ((lambda **k: LinkAccumulator(cfg, "cpu", seed, **k), lambda a: a.errors.numpy()),
                           (lambda **k: RateAccumulator(cfg, "cpu", seed, (1.0, 0.5), 0.01, **k), lambda a: a.loss.numpy()),
                           (lambda **k: BlockErrorAccumulator(code, "cpu", seed, 0.01, **k), lambda a: a.errors.numpy())):
            a, b = make(**kw), make(**kw, precoding_subband=None)
            for pilots, ideal, meta in batches:
                a.update(model(pilots), ideal, meta)
                b.update(model(pilots), ideal, meta)
            assert a.frames == b.frames and b.precoding_subband is None and np.array_equal(read(a), read(b)), kw
            assert type(a._plan) is type(b._plan) and not hasattr(b, "_pmi_counts")


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    import ctypes as C
    assert _abi.AFT_ABI_VERSION == 10 and _abi.AFT_LINK_MAX_SUBBANDS == 1024
    restype, argtypes = _abi.SIGNATURES["aft_link_precoded_f32"]
    assert "aft_link_precoded_f32" in _abi.EXPORTED_SYMBOLS and restype is C.c_int and len(argtypes) == 17
    assert argtypes[0]._type_ is _abi.AftLink and [i for i, t in enumerate(argtypes) if t is C.c_int] == [8, 9, 10, 15]
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_precoded_f32") == names.index("aft_link_alamouti_f32") + 1            # the header's order


# ---- the conditions on the inputs the GPU tests use ----

def test_the_pmi_flagged_subbands_on_the_inputs_the_gpu_tests_use():
    """At PMI_TAU_CAP every case has at most ONE PMI-flagged subband and the small grids have none.  The smallest gaps relative to
    ``Gr_b`` are printed: conditions, not measurements."""
    smallest = {"small": (np.inf, None), "large": (np.inf, None), "second": (np.inf, None)}
    for name, R, n, B in pc_cases():
        for which in ("lmmse", "ideal"):
            sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R, which)
            cfg = LinkConfig(sim, 4)
            pmi, flags = precoding_pmi_host(cfg, est, rho, R, B, PMI_TAU_CAP)
            assert pmi.shape == flags.shape == (n // (2 * R), -(-sim.ofdm[0] // B)) and pmi.min() >= 0 and pmi.max() <= 3
            assert flags.sum() <= (0 if name in SMALL else 1), (name, R, B, which, int(flags.sum()))
            # the gap itself: the largest tau at which nothing is flagged, by bisection on the documented condition
            lo, hi = 0.0, 4.0
            for _ in range(60):
                mid = (lo + hi) / 2
                lo, hi = (lo, mid) if precoding_pmi_host(cfg, est, rho, R, B, mid)[1].any() else (mid, hi)
            kind = "small" if name in SMALL else "large"
            if hi < smallest[kind][0]:
                if kind == "large":
                    smallest["second"] = smallest["large"]
                smallest[kind] = (hi, (name, R, B, which))
            elif kind == "large" and hi < smallest["second"][0]:
                smallest["second"] = (hi, (name, R, B, which))
    print(f"smallest gap / Gr_b: {smallest['large'][0]:.2e} at {smallest['large'][1]}, then {smallest['second'][0]:.2e} at "
          f"{smallest['second'][1]}; on the small grids {smallest['small'][0]:.2e} at {smallest['small'][1]}")
    assert smallest["small"][0] > PMI_TAU_CAP


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_flagged_share_on_the_inputs_the_gpu_tests_use(m):
    """At TAU_CAP: at most 1e-3 of the data (element, axis) pairs on the two large grids, and at most one flagged (element, axis) per
    case on the two small ones, where one flag alone is 3e-3 of the pairs.  Conditions, not measurements."""
    worst, most = (0.0, None), 0
    for name, R, _, B in pc_cases():
        for which in ("lmmse", "ideal"):
            sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R, which)
            cfg = LinkConfig(sim, m)
            flags = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, tau=TAU_CAP)[4]
            if name in LARGE:
                share = flagged_share(cfg, flags)
                assert share <= SHARE_CAP, (name, R, B, which, share)
                if share >= worst[0]:
                    worst = (share, (name, R, B, which))
            else:
                assert flags.sum() <= 1, (name, R, B, which, int(flags.sum()))
                most = max(most, int(flags.sum()))
    print(f"m = {m}: the largest flagged share at TAU_CAP is {worst[0]:.2e} at {worst[1]}; at most {most} flag on the small grids")


def test_the_kernel_spills_no_vector_register():
    """hipcc's own resource report of k_linkprecode.hip: ``VGPRs Spill: 0`` for the four instantiations."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adafortitran_amd", "csrc")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "k_linkprecode.hip", "-o",
                          "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    report, name = {}, None
    for line in res.stderr.splitlines():
        found = re.search(r"Function Name: (\S+)", line)
        if found:
            name = found.group(1)
        found = re.search(r"VGPRs Spill: (\d+)", line)
        if found and name:
            report[name] = int(found.group(1))
    kernels = {k: v for k, v in report.items() if "link_precoded_kernel" in k}
    assert len(kernels) == 4 and all(v == 0 for v in kernels.values()), report
