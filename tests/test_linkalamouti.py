"""``linksim``'s transmit-diversity link on the CPU: ``alamouti_pairs`` on a grid whose pairs straddle pilots and its invariants on every
grid, ``link_alamouti_host`` at the exact extremes, against a brute force over all ``2^m`` symbols on a combiner rebuilt pair by pair
from the documented streams, an unheard second antenna against the diversity link, the lone elements, the orthogonality of a pair
under a constant channel, the refusals, the four accumulators and the three sweeps of ``evaluation`` with ``tx_diversity=`` against
the definition applied batch by batch, the binding, the share of flagged decisions on the inputs tests/test_linkalamouti_gpu.py
compares the kernel on, and the compiler's register report of the kernel.

``al_inputs`` builds those inputs once per grid: tests/test_linksm.py's three grids and ``straddle_9x6``, whose lines begin and end with
a pilot, which has a time pair (t = 1, 3) across a pilot, a frequency pair (s = 1, 4) across two adjacent pilots and lone elements
in both pairings.  The GPU file imports it, so both files speak about the same arrays."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, simulate_frames_host, words
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, PAIRINGS, BlockErrorAccumulator, CodeConfig, HarqAccumulator,
                                      LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator,
                                      alamouti_pairs, alamouti_weights, branch_weights, constellation, link_alamouti_host,
                                      link_decode_host, link_ldpc_host, link_mrc_host, llr_scale, noise_sigma)
from adafortitran_amd.lmmse import lmmse_estimate_host
from test_linkmrc import MRC_ODD
from test_linksim import GRIDS, SEED, SHARE_CAP, TAU_CAP, flagged_share
from test_linksm import SM_GRIDS, sm_inputs

STRADDLE = "straddle_9x6"
STRADDLE_SIM = ChannelSimConfig(ofdm=(9, 6), pilot=(4, 3), pilot_scs=(0, 2, 3, 8), pilot_symbols=(0, 2, 5))
AL_GRIDS = {**SM_GRIDS, STRADDLE: 16}                           # frames [0, n) of seed 3
LARGE, SMALL = ("default_120x14", "odd_30x7"), (MRC_ODD, STRADDLE)
BRANCHES = (1, 2, 3, 4, 8)
_straddle = []


def al_inputs(name):
    """``test_linksm.sm_inputs``' tuple (sim, keys, sigma, snr, ideal, {"lmmse": .., "ideal": ..}) for its three grids, and the same
    recipe on ``straddle_9x6``; made once, read-only."""
    if name != STRADDLE:
        return sm_inputs(name)
    if not _straddle:
        sim, n = STRADDLE_SIM, AL_GRIDS[STRADDLE]
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(n))
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        est = {"lmmse": lmmse_estimate_host(sim, pilots, meta).astype(np.complex64), "ideal": ideal}
        keys, sigma, snr = frame_keys(SEED, np.arange(n)), noise_sigma(meta[:, 0]), meta[:, 0].astype(np.float64)
        for a in (ideal, est["lmmse"], keys, sigma, snr):
            a.setflags(write=False)
        _straddle.append((sim, keys, sigma, snr, ideal, est))
    return _straddle[0]


def al_cases():
    """(grid, R, frames used): every R whose groups of 2 R frames fit into the grid's frames, on the frames they fill."""
    return [(name, R, n // (2 * R) * 2 * R) for name, n in AL_GRIDS.items() for R in BRANCHES if n >= 2 * R]


def al_operands(name, R, which="lmmse", err_var=0.0):
    sim, keys, sigma, snr, ideal, est = al_inputs(name)
    n = len(keys) // (2 * R) * 2 * R
    rho, scale = alamouti_weights(snr[:n], err_var, R)
    return sim, n, keys[:n], sigma[:n], ideal[:n], est[which][:n], rho, scale


# ---- the pairs ----

def test_the_pairs_of_the_straddle_grid():
    cfg = LinkConfig(STRADDLE_SIM, 4)
    role, partner = alamouti_pairs(cfg, "time")
    assert role.dtype == np.int8 and partner.dtype == np.int64 and role.shape == partner.shape == (9, 6)
    for s in range(9):
        assert role[s].tolist() == ([-1, 0, -1, 1, 2, -1] if s in (0, 2, 3, 8) else [0, 1, 0, 1, 0, 1]), s
    assert partner[0, 1] == 3 and partner[0, 3] == 1 and partner[0, 4] == 4 and partner[0, 0] == 0      # the pair (t = 1, 3) across a pilot
    assert partner[1].tolist() == [7, 6, 9, 8, 11, 10]
    role, partner = alamouti_pairs(cfg, "frequency")
    for t in range(6):
        assert role[:, t].tolist() == ([-1, 0, -1, -1, 1, 0, 1, 2, -1] if t in (0, 2, 5) else [0, 1, 0, 1, 0, 1, 0, 1, 2]), t
    assert partner[1, 0] == 4 * 6 and partner[4, 0] == 1 * 6 and partner[7, 0] == 7 * 6                 # the pair (s = 1, 4) across two pilots
    assert partner[8, 1] == 8 * 6 + 1 and partner[0, 1] == 6 + 1
    assert PAIRINGS == ("time", "frequency")
    for bad in ("space", "Time", None, 0):
        with pytest.raises(ValueError, match="pairing"):
            alamouti_pairs(cfg, bad)


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_the_pairs_on_every_grid(pairing):
    """``partner`` is an involution, a first precedes its second on the same line with only pilots between them, and a line has at
    most one lone element, its last data element."""
    sims = {**{name: sim for name, (sim, _) in GRIDS.items()}, STRADDLE: STRADDLE_SIM}
    assert "pilot_bounds_128x40" in sims
    for name, sim in sims.items():
        cfg = LinkConfig(sim, 2)
        S, T = sim.ofdm
        role, partner = alamouti_pairs(cfg, pairing)
        flat, mask = partner.reshape(-1), cfg.data_mask
        assert np.array_equal(flat[flat], np.arange(S * T)), name
        assert np.array_equal(role >= 0, mask) and np.array_equal(partner == np.arange(S * T).reshape(S, T), (role == -1) | (role == 2))
        assert (role.reshape(-1)[flat[role.reshape(-1) == 0]] == 1).all() and (role.reshape(-1)[flat[role.reshape(-1) == 1]] == 0).all()
        step = 1 if pairing == "time" else T                                     # the flat distance of neighbours on a line
        lines_r, lines_m = (role, mask) if pairing == "time" else (role.T, mask.T)
        for q in np.flatnonzero(role.reshape(-1) == 0):
            b = flat[q]
            assert b > q and (b - q) % step == 0, (name, q)
            assert (q // T == b // T) if pairing == "time" else (q % T == b % T)
            assert not mask.reshape(-1)[q + step:b:step].any(), (name, q)       # only pilots between a and b
        for r, msk in zip(lines_r, lines_m):
            data = r[msk]
            assert (data == 2).sum() == len(data) % 2 and (len(data) % 2 == 0 or data[-1] == 2), name
            assert data[:len(data) // 2 * 2].tolist() == [0, 1] * (len(data) // 2)


# ---- the definition ----

def _constant_channels(n, S, T, seed=7):
    rng = np.random.default_rng(seed)
    h = (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2.0) + 0.2
    return np.broadcast_to(h.astype(np.complex64)[:, None, None], (n, S, T)).copy()


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_exact_extremes(m, pairing):
    """One constant per frame as the channel, the estimates are the channels and there is no noise: the pairs are orthogonal, no bit is
    wrong and no decision is flagged.  Estimates that point the other way flip every bit at m = 2."""
    for name, R, n in al_cases():
        sim, n, keys, sigma, _, _, rho, scale = al_operands(name, R)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        H, zero = _constant_channels(n, *sim.ofdm), np.zeros_like(sigma)
        counts, loss, llr, wrong, flags = link_alamouti_host(cfg, keys, H, H, zero, rho, scale, R, pairing, tau=TAU_CAP)
        assert counts.shape == (G, 2) and counts.dtype == np.int64 and loss.shape == (G, 1) and llr.shape == (G, *sim.ofdm, m)
        assert wrong.shape == (G, *sim.ofdm) and flags.shape == (G, *sim.ofdm, 2)
        assert not counts.any() and not wrong.any() and not flags.any(), (name, R)
        assert not llr[:, ~cfg.data_mask].any() and (llr[:, cfg.data_mask] != 0).all()
        if m == 2:
            counts, _, _, _, flags = link_alamouti_host(cfg, keys, H, -H, zero, rho, scale, R, pairing, tau=TAU_CAP)
            assert (counts[:, 0] == 2 * cfg.data_elements).all() and (counts[:, 1] == cfg.data_elements).all() and not flags.any()


def _rebuilt(cfg, keys, ideal, est, sigma, rho, R, pairing):
    """(x [G,S,T], c [G,S,T], p [G,S,T]) as the module docstring writes them, pair by pair in plain loops over the lines, from the
    documented streams: float64, independent of ``alamouti_pairs``."""
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
    c, p = np.zeros((G, S, T), complex), np.zeros((G, S, T))
    mask = cfg.data_mask
    lines = [[(s, t) for t in range(T) if mask[s, t]] for s in range(S)] if pairing == "time" else \
        [[(s, t) for s in range(S) if mask[s, t]] for t in range(T)]
    for line in lines:
        for i in range(0, len(line) - 1, 2):
            a, b = line[i], line[i + 1]
            for r in range(R):
                h0a, h1a, h0b, h1b = H[:, r, 0][:, a[0], a[1]], H[:, r, 1][:, a[0], a[1]], H[:, r, 0][:, b[0], b[1]], H[:, r, 1][:, b[0], b[1]]
                e0a, e1a, e0b, e1b = E[:, r, 0][:, a[0], a[1]], E[:, r, 1][:, a[0], a[1]], E[:, r, 0][:, b[0], b[1]], E[:, r, 1][:, b[0], b[1]]
                xa, xb = x[:, a[0], a[1]], x[:, b[0], b[1]]
                ya = h0a * xa + h1a * xb + noise[:, r, a[0], a[1]]
                yb = -h0b * xb.conj() + h1b * xa.conj() + noise[:, r, b[0], b[1]]
                c[:, a[0], a[1]] += w[:, r] * (e0a.conj() * ya + e1b * yb.conj())
                c[:, b[0], b[1]] += w[:, r] * (e1a.conj() * ya - e0b * yb.conj())
                p[:, a[0], a[1]] += w[:, r] * (np.abs(e0a) ** 2 + np.abs(e1b) ** 2)
                p[:, b[0], b[1]] += w[:, r] * (np.abs(e1a) ** 2 + np.abs(e0b) ** 2)
        if len(line) % 2:
            s, t = line[-1]
            for r in range(R):
                y = H[:, r, 0][:, s, t] * x[:, s, t] + noise[:, r, s, t]
                c[:, s, t] += w[:, r] * (E[:, r, 0][:, s, t].conj() * y)
                p[:, s, t] += w[:, r] * np.abs(E[:, r, 0][:, s, t]) ** 2
    return x, c, p


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


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_llrs_against_a_brute_force_over_all_symbols(m, pairing):
    """``scale |c - p a|^2 / p`` over all 2^m symbols on the combiner rebuilt pair by pair: pins the pairs, the signs and conjugates of
    the code, the weights, the separable form, the bit order and the leader's scale, to 1e-9 q."""
    for name, R in ((STRADDLE, 1), (STRADDLE, 2), ("odd_30x7", 3), (MRC_ODD, 2)):
        sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R, "lmmse", 0.01)
        cfg = LinkConfig(sim, m)
        out = link_alamouti_host(cfg, keys, ideal, est, sigma, rho, scale, R, pairing, e_lambda=TAU_CAP)
        llr, q = out[2], out[5]
        _, c, p = _rebuilt(cfg, keys, ideal, est, sigma, rho, R, pairing)
        want = _brute_force(cfg, c, p, scale)
        assert llr.shape == want.shape == q.shape == (n // (2 * R), *sim.ofdm, m)
        assert (np.abs(llr - want) <= 1e-9 * q).all(), (name, R, float((np.abs(llr - want) / np.where(q > 0, q, 1)).max()))
        assert (q[:, cfg.data_mask] > 0).all() and (q[:, ~cfg.data_mask] == 0).all()


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_antenna_is_the_diversity_link(m, pairing):
    """``H_r1 = E_r1 = 0``: at first and lone elements the wrong bits are ``link_mrc_host``'s on the frames (r, 0) and the LLRs equal
    it exactly -- the second term of every sum is an exact zero."""
    for name, R, n in al_cases():
        sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R)
        cfg = LinkConfig(sim, m)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        _, _, llr, wrong, _ = link_alamouti_host(cfg, keys, H, E, sigma, rho, scale, R, pairing, tau=TAU_CAP)
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R, tau=TAU_CAP)
        role = alamouti_pairs(cfg, pairing)[0]
        heard = (role == 0) | (role == 2)
        assert heard.any() and np.array_equal(wrong[:, heard], want[3][:, heard]), (name, R)
        assert np.array_equal(llr[:, heard], want[2][:, heard]), (name, R)


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_lone_elements_do_not_hear_the_second_antenna(pairing):
    for name, R in ((STRADDLE, 2), (MRC_ODD, 2), ("odd_30x7", 4)):
        sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R)
        cfg = LinkConfig(sim, 6)
        lone = alamouti_pairs(cfg, pairing)[0] == 2
        assert lone.any()
        rng = np.random.default_rng(11)
        H, E = ideal.copy(), est.copy()
        H[1::2] = (rng.normal(size=H[1::2].shape) + 1j * rng.normal(size=H[1::2].shape)).astype(np.complex64)
        E[1::2] = (rng.normal(size=E[1::2].shape) - 1j * rng.normal(size=E[1::2].shape)).astype(np.complex64)
        got = link_alamouti_host(cfg, keys, H, E, sigma, rho, scale, R, pairing, tau=TAU_CAP)
        want = link_alamouti_host(cfg, keys, ideal, est, sigma, rho, scale, R, pairing, tau=TAU_CAP)
        assert np.array_equal(got[2][:, lone], want[2][:, lone]) and np.array_equal(got[3][:, lone], want[3][:, lone])
        assert not np.array_equal(got[2][:, ~lone], want[2][:, ~lone])


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_a_pair_is_orthogonal_under_a_constant_channel(pairing):
    """``E = H`` and ``H`` equal at a and b: ``c - p x`` is the noise's share alone, so it does not move when the sent words do.  At
    m = 2 an axis's LLR is ``-4 d scale comp``, which is how ``c`` is read off the definition; the leader's own noise is switched off
    so that a second leader key changes every sent word and no noise.  With the simulated channel, which varies inside a pair, the
    same residual does move."""
    R, name = 2, STRADDLE
    sim, n, keys, sigma, ideal, _, rho, _ = al_operands(name, R)
    cfg, W = LinkConfig(sim, 2), 2 * R
    G = n // W
    scale = np.full(G, 2.0, np.float32)
    sigma = sigma.copy()
    sigma[::W] = 0
    other = keys.copy()
    other[::W] = frame_keys(SEED + 1, np.arange(G))
    mask = cfg.data_mask
    const = _constant_channels(n, *sim.ofdm)

    def residual(H, k):
        llr = link_alamouti_host(cfg, k, H, H, sigma, rho, scale, R, pairing)[2]
        c = -(llr[..., 0] + 1j * llr[..., 1]) / (4 * cfg.d * 2.0)
        x, _, p = _rebuilt(cfg, k, H, H, sigma, rho, R, pairing)
        return (c - p * x)[:, mask], x[:, mask], np.abs(p[:, mask]).max()

    r0, x0, size = residual(const, keys)
    r1, x1, _ = residual(const, other)
    assert (x0 != x1).mean() > 0.5 and np.abs(r0).max() > 1e-3 * size            # other words; a residual that is not trivially zero
    assert np.abs(r0 - r1).max() <= 1e-12 * size
    v0, v1 = residual(ideal, keys)[0], residual(ideal, other)[0]
    assert np.abs(v0 - v1).max() > 1e-6 * size                                    # the cross-talk this link exists to measure


def test_the_weights():
    snr = np.array([0.0, 25.0, 10.0, 10.0, 30.0, 5.0, 7.0, 7.0])
    for err_var in (0.0, 0.02):
        rho, scale = alamouti_weights(snr, err_var, 2)
        assert rho.dtype == scale.dtype == np.float32 and rho.shape == (8,) and scale.shape == (2,)
        assert scale.tobytes() == llr_scale(snr, err_var)[::4].tobytes() and rho.tobytes() == branch_weights(snr, err_var, 4)[0].tobytes()
    assert alamouti_weights(snr, 0.0, 4)[1].shape == (1,) and alamouti_weights(snr, 0.0, 1)[1].shape == (4,)


def test_refusals():
    sim, n, keys, sigma, ideal, est, rho, scale = al_operands("odd_30x7", 4)
    cfg = LinkConfig(sim, 4)
    code = CodeConfig(cfg, 64)
    for bad in ("space", "TIME", None, 1, True):
        with pytest.raises(ValueError, match="pairing"):
            link_alamouti_host(cfg, keys, ideal, est, sigma, rho, scale, 4, bad)
    for bad in ("space", "TIME", 1, True):
        for make in (lambda: LinkAccumulator(cfg, "cpu", tx_diversity=bad), lambda: RateAccumulator(cfg, "cpu", tx_diversity=bad),
                     lambda: BlockErrorAccumulator(code, "cpu", tx_diversity=bad)):
            with pytest.raises(ValueError, match="pairing"):
                make()
    for bad in (0, 9, 2.0, -1, True, "2"):
        with pytest.raises(ValueError, match="branches"):
            link_alamouti_host(cfg, keys, ideal, est, sigma, rho, scale, bad)
        with pytest.raises(ValueError, match="branches"):
            alamouti_weights(np.zeros(16), 0.0, bad)
        with pytest.raises(ValueError, match="branches"):
            LinkAccumulator(cfg, "cpu", branches=bad, tx_diversity="time")
    with pytest.raises(ValueError, match="32 frames is not a multiple of branches \\* 2 = 3 \\* 2"):
        link_alamouti_host(cfg, keys, ideal, est, sigma, rho, scale, 3)
    with pytest.raises(ValueError, match="6 frames is not a multiple of branches \\* 2 = 2 \\* 2"):
        alamouti_weights(np.zeros(6), 0.0, 2)
    with pytest.raises(ValueError, match="rho"):
        link_alamouti_host(cfg, keys, ideal, est, sigma, rho[:8], scale, 4)
    with pytest.raises(ValueError, match="scale"):
        link_alamouti_host(cfg, keys, ideal, est, sigma, rho, scale[:3], 4)
    for make in (lambda: LinkAccumulator(cfg, "cpu", branches=2, streams=2, tx_diversity="time"),
                 lambda: RateAccumulator(cfg, "cpu", branches=2, streams=2, tx_diversity="frequency"),
                 lambda: BlockErrorAccumulator(code, "cpu", branches=2, streams=2, tx_diversity="time"),
                 lambda: LdpcBlockErrorAccumulator(LdpcConfig(cfg, (3, 6)), "cpu", branches=2, streams=2, tx_diversity="time")):
        with pytest.raises(ValueError, match="tx_diversity.*streams must be 1"):
            make()
    LinkAccumulator(cfg, "cpu", detector="anything", tx_diversity="time")        # the detector is ignored
    for make in (lambda: LinkAccumulator(cfg, "cpu", branches=2, tx_diversity="time"),
                 lambda: RateAccumulator(cfg, "cpu", branches=2, tx_diversity="frequency"),
                 lambda: BlockErrorAccumulator(code, "cpu", branches=2, tx_diversity="time")):
        with pytest.raises(ValueError, match="6 frames is not a multiple of branches \\* 2 = 2 \\* 2"):
            make().update(None, torch.from_numpy(ideal[:6].copy()), frame_ids=np.arange(6), snr_db=np.zeros(6))
    import inspect
    assert "tx_diversity" not in inspect.signature(HarqAccumulator.__init__).parameters
    for cls in (LinkAccumulator, RateAccumulator, BlockErrorAccumulator, LdpcBlockErrorAccumulator):
        par = inspect.signature(cls.__init__).parameters["tx_diversity"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY


class _Ls(torch.nn.Module):
    """The LS-interpolated estimate as a model ``evaluation.forward_pass`` can call."""

    def __init__(self, sim):
        super().__init__()
        self.sim = sim
        self.register_buffer("anchor", torch.zeros(1))

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.numpy()))


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_accumulators_and_sweeps_with_transmit_diversity_on_the_host(pairing):
    """A host ``SynthLoader`` (every frame at its own SNR), three batches of eight frames (two groups of 2 x 2): each accumulator and
    each sweep equals the definition applied batch by batch, the coded ones through the host decoders on the definition's LLRs rounded
    to float32 with the leaders' keys."""
    from adafortitran_amd.evaluation import get_link_bler, get_link_rates, get_link_stats
    R, seed, err_var = 2, 5, 0.01
    sim = GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code, ldpc = CodeConfig(cfg, 64, "1/2"), LdpcConfig(cfg, (3, 6))
    factors = (1.0, 0.5)
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 8, 24, device="cpu", seed=seed))
    assert len(batches) == 3
    kw = dict(branches=R, tx_diversity=pairing)
    hard, rate = LinkAccumulator(cfg, "cpu", seed, **kw), RateAccumulator(cfg, "cpu", seed, factors, err_var, **kw)
    conv, lay = BlockErrorAccumulator(code, "cpu", seed, err_var, **kw), LdpcBlockErrorAccumulator(ldpc, "cpu", seed, err_var, **kw)
    want = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "loss0": np.zeros(8), "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64),
            "conv0": np.zeros(2, np.int64)}
    for pilots, ideal, meta in batches:
        est = model(pilots)
        for acc in (hard, rate, conv, lay):
            acc.update(est, ideal, meta)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        lead = np.ascontiguousarray(keys[::2 * R])
        snr = meta[1].numpy().reshape(-1)
        for ev, tag in ((0.0, "0"), (err_var, "")):
            rho, scale = alamouti_weights(snr, ev, R)
            counts, loss, llr = link_alamouti_host(cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), rho, scale, R, pairing,
                                                   factors if tag == "" else np.asarray([2.0 ** -k for k in range(8)]))
            if tag == "0":
                want["hard"] += counts.sum(axis=0)
                want["loss0"] += loss.sum(axis=0)
                want["conv0"] += link_decode_host(code, lead, llr.astype(np.float32))[0].sum(axis=0)
            else:
                want["loss"] += loss.sum(axis=0)
                want["conv"] += link_decode_host(code, lead, llr.astype(np.float32))[0].sum(axis=0)
                want["ldpc"] += link_ldpc_host(ldpc, lead, llr.astype(np.float32))[0].sum(axis=0)
    F = 6                                                                        # frames counts the groups
    assert hard.frames == rate.frames == conv.frames == lay.frames == F and hard.tx_diversity == pairing
    assert hard.errors.tolist() == want["hard"].tolist() and hard.result() == want["hard"][0] / (F * cfg.bits_per_frame)
    assert hard.result_ser() == want["hard"][1] / (F * cfg.data_elements)
    assert np.array_equal(rate.loss.numpy(), want["loss"])
    assert rate.result() == [4 - v / (F * cfg.data_elements) for v in want["loss"]]
    assert conv.errors.tolist() == want["conv"].tolist() and conv.result() == want["conv"][1] / (F * code.blocks)
    assert lay.errors.tolist() == want["ldpc"].tolist() and lay.result() == want["ldpc"][1] / (F * ldpc.blocks)
    assert 0 < want["hard"][0] < F * cfg.bits_per_frame // 2                       # the frames are not trivial
    loaders = [("SNR_0", SynthLoader(sim, 8, 24, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_stats(model, loaders, cfg, seed, **kw) == {0: want["hard"][0] / (F * cfg.bits_per_frame)}
    assert get_link_rates(model, loaders, cfg, seed, **kw) == {0: max(4 - v / (F * cfg.data_elements) for v in want["loss0"])}
    assert get_link_bler(model, loaders, code, seed, **kw) == {0: want["conv0"][1] / (F * code.blocks)}
    assert get_link_bler(model, loaders, ldpc, seed, err_var, **kw) == {0: want["ldpc"][1] / (F * ldpc.blocks)}
    with pytest.raises(ValueError, match="streams must be 1"):
        get_link_stats(model, loaders, cfg, seed, branches=R, streams=2, tx_diversity=pairing)


def test_without_transmit_diversity_the_objects_are_todays():
    seed, sim = 5, GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 4, 8, device="cpu", seed=seed))
    for R in (1, 2):
        a, b = LinkAccumulator(cfg, "cpu", seed, R), LinkAccumulator(cfg, "cpu", seed, R, tx_diversity=None)
        for pilots, ideal, meta in batches:
            a.update(model(pilots), ideal, meta)
            b.update(model(pilots), ideal, meta)
        assert a.frames == b.frames == 8 // R and b.tx_diversity is None and a.errors.tolist() == b.errors.tolist()


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    import ctypes as C
    assert _abi.AFT_ABI_VERSION == 10 and _abi.AFT_LINK_PAIR_TIME == 0 and _abi.AFT_LINK_PAIR_FREQUENCY == 1
    restype, argtypes = _abi.SIGNATURES["aft_link_alamouti_f32"]
    assert "aft_link_alamouti_f32" in _abi.EXPORTED_SYMBOLS and restype is C.c_int and len(argtypes) == 16
    assert argtypes[0]._type_ is _abi.AftLink and [i for i, t in enumerate(argtypes) if t is C.c_int] == [8, 9, 10, 14]
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_alamouti_f32") == names.index("aft_link_joint_f32") + 1               # the header's order


# ---- the flagged share on the inputs the GPU tests use ----

@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_flagged_share_on_the_inputs_the_gpu_tests_use(m):
    """At TAU_CAP: at most 1e-3 of the data (element, axis) pairs on the two large grids, and at most one flagged (element, axis) per
    case on the two small ones, where one flag alone is 3e-3 of the pairs.  Conditions, not measurements."""
    worst, most = (0.0, None), 0
    for name, R, _ in al_cases():
        for pairing in PAIRINGS:
            for which in ("lmmse", "ideal"):
                sim, n, keys, sigma, ideal, est, rho, scale = al_operands(name, R, which)
                cfg = LinkConfig(sim, m)
                flags = link_alamouti_host(cfg, keys, ideal, est, sigma, rho, scale, R, pairing, tau=TAU_CAP)[4]
                if name in LARGE:
                    share = flagged_share(cfg, flags)
                    assert share <= SHARE_CAP, (name, R, pairing, which, share)
                    if share >= worst[0]:
                        worst = (share, (name, R, pairing, which))
                else:
                    assert flags.sum() <= 1, (name, R, pairing, which, int(flags.sum()))
                    most = max(most, int(flags.sum()))
    print(f"m = {m}: the largest flagged share at TAU_CAP is {worst[0]:.2e} at {worst[1]}; at most {most} flag on the small grids")


def test_the_kernel_spills_no_vector_register():
    """hipcc's own resource report of k_linkalamouti.hip: ``VGPRs Spill: 0`` for every instantiation (four modulation orders, two
    pairings)."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adafortitran_amd", "csrc")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "k_linkalamouti.hip", "-o",
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
    kernels = {k: v for k, v in report.items() if "link_alamouti_kernel" in k}
    assert len(kernels) == 8 and all(v == 0 for v in kernels.values()), report
