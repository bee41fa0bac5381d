"""Delayed PMI feedback on the closed-loop link (adafortitran_amd/linksim.py, "delayed feedback") on the CPU, no library needed:
``link_precoded_host(..., slots=K, delay=d)`` and ``precoding_pmi_host`` against the instantaneous definition -- ``delay=0`` bit for bit
for any ``slots``, estimates made equal across a sequence's slots bit for bit on the transmit groups, the applied PMIs the selection on
the feedback groups, the compact output rows written out index by index at ``K=3, d=2`` and ``K=2, d=1`` --, the refusals, the four
accumulators and the three sweeps of ``evaluation`` with ``precoding_delay=`` against the definition applied batch by batch, and the
orderings a stale precoder must show on the twins with perfect channel knowledge.

The inputs (``delay_inputs``, shared with tests/test_linkprecode_delay_gpu.py) are 24 frames of seed 3 from a simulator with
``slots=3, antennas=(2, 2)``: two sequences of three slots at R = 2, four at R = 1 (the layout ``g 2R + r 2 + s`` is the simulator's
for R = 2; for R = 1 the same frames are read as groups of two, which the bit comparisons do not mind).  The SNR of a frame is its
sequence's plus an offset by its antenna (``EQUAL_SNR``: the same in every slot, so ``rho`` repeats across a sequence's slots) or by its
frame number (``MIXED_SNR``: ``rho`` differs from slot to slot, so the feedback group's weights are seen to be the ones the selection
reads).

The orderings.  2 x 1 with perfect channel knowledge, QPSK at 10 dB, slots of 2 symbols (``ofdm=(24, 2)``) so that one slot of delay
is 2 symbols: at the top Doppler bin (1400 Hz, 0.1 turns per symbol) the channel's autocorrelation J0(2 pi 0.1 2 d) is 0.64 at d = 1
and -0.17 at d = 4, so the precoder chosen d slots ago is partly right at d = 1 and unrelated at d = 4, where a random choice among
four differs from the slot's own with probability 3/4.  400 sequences of 5 slots, 6 subbands each: at d = 4 the share's standard error
is below 0.01, and the shares measured here on the twins (printed) are 0.57 and 0.77, twenty standard errors apart; the bit errors
on the slots every delay sends are 139 at d = 0 and 963 at d = 4.  At 0 Hz the rays do not move
and the estimates (the channel itself) are equal in every slot: the stale share is exactly 0."""
import numpy as np
import pytest
import torch

from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, simulate_frames_host
from adafortitran_amd.evaluation import get_link_bler, get_link_rates, get_link_stats
from adafortitran_amd.linksim import (BlockErrorAccumulator, CodeConfig, HarqAccumulator, LdpcBlockErrorAccumulator, LdpcConfig,
                                      LinkAccumulator, LinkConfig, RateAccumulator, delayed_groups, link_decode_host, link_ldpc_host,
                                      link_precoded_host, noise_sigma, precoding_pmi_host, precoding_weights)
from adafortitran_amd.lmmse import lmmse_estimate_host
from test_linkmrc import MRC_ODD
from test_linksim import TAU_CAP

SEED = 3
DELAY_SIMS = {"odd_30x7": ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3), slots=3, antennas=(2, 2), rx_correlation=0.3),
              MRC_ODD: ChannelSimConfig(ofdm=(3, 5), pilot=(1, 1), slots=3, antennas=(2, 2), rx_correlation=0.3)}
FRAMES = 24
EQUAL_SNR, MIXED_SNR = "equal", "mixed"
_inputs = {}


def delay_inputs(name):
    """(sim, keys uint64 [24], {"equal" | "mixed": (sigma float32, snr float64)}, ideal complex64, est complex64 -- the LMMSE estimate):
    made once per grid, read-only."""
    if name not in _inputs:
        sim = DELAY_SIMS[name]
        g = np.arange(FRAMES)
        ideal, pilots, meta = simulate_frames_host(sim, SEED, g)
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        est = lmmse_estimate_host(sim, pilots, meta).astype(np.complex64)
        base = meta[:, 0].astype(np.float64)
        snr = {EQUAL_SNR: base + 1.5 * (g % 4), MIXED_SNR: base + 0.7 * (g % 5) + 0.4 * (g % 4)}
        noise = {k: (noise_sigma(v), v) for k, v in snr.items()}
        keys = frame_keys(SEED, g)
        for a in (ideal, est, keys, *(x for pair in noise.values() for x in pair)):
            a.setflags(write=False)
        _inputs[name] = (sim, keys, noise, ideal, est)
    return _inputs[name]


def delay_operands(name, R, which=MIXED_SNR, err_var=0.0):
    """(cfg's sim, keys, sigma, ideal, est, rho, scale) for the 24 frames."""
    sim, keys, noise, ideal, est = delay_inputs(name)
    sigma, snr = noise[which]
    return (sim, keys, sigma, ideal, est, *precoding_weights(snr, err_var, R))


def equal_estimates(est, R, K):
    """The estimates with every slot of a sequence given slot 0's: ``[Q, K, 2R, S, T]`` with the K axis overwritten."""
    e = est.reshape(-1, K, 2 * R, *est.shape[1:]).copy()
    e[:, 1:] = e[:, :1]
    return e.reshape(est.shape)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


CASES = [(name, R, m, B) for name in DELAY_SIMS for R in (1, 2) for m in (2, 6) for B in (1, 7, None)]


def _band(name, B):
    S = DELAY_SIMS[name].ofdm[0]
    return S if B is None else min(B, S)


def test_the_output_groups():
    sent, feedback = delayed_groups(6, 3, 2)
    assert sent.tolist() == [2, 5] and feedback.tolist() == [0, 3] and sent.dtype == np.int64
    sent, feedback = delayed_groups(6, 2, 1)
    assert sent.tolist() == [1, 3, 5] and feedback.tolist() == [0, 2, 4]
    sent, feedback = delayed_groups(6, 3, 1)
    assert sent.tolist() == [1, 2, 4, 5] and feedback.tolist() == [0, 1, 3, 4]
    sent, feedback = delayed_groups(4, 1, 0)
    assert sent.tolist() == feedback.tolist() == [0, 1, 2, 3]
    for groups, K, d in ((6, 4, 1), (6, 3, 3), (6, 3, -1), (6, 0, 0), (6, 3.0, 1), (6, 3, True)):
        with pytest.raises(ValueError):
            delayed_groups(groups, K, d)


@pytest.mark.parametrize("name,R,m,B", CASES)
def test_no_delay_is_the_instantaneous_link_bit_for_bit(name, R, m, B):
    sim, keys, sigma, ideal, est, rho, scale = delay_operands(name, R)
    cfg, B = LinkConfig(sim, m), _band(name, B)
    want = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, (1.0, 0.5))
    for K in (1, 2, 3) if R == 1 else (1, 3):
        _same(link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, (1.0, 0.5), slots=K, delay=0), want)
        assert np.array_equal(precoding_pmi_host(cfg, est, rho, R, B, slots=K, delay=0), want[3])
    full = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, tau=TAU_CAP, e_lambda=TAU_CAP)
    _same(link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, tau=TAU_CAP, e_lambda=TAU_CAP, slots=3, delay=0), full)


@pytest.mark.parametrize("name,R,m,B", CASES)
def test_equal_estimates_across_slots_give_the_instantaneous_link_on_the_transmit_groups(name, R, m, B):
    """The estimates and rho of every slot of a sequence are slot 0's, the true channels are left different: the PMIs selected d slots
    ago are the slot's own, so delay d is the instantaneous link on the transmit groups' frames, bit for bit."""
    sim, keys, sigma, ideal, est, rho, scale = delay_operands(name, R, EQUAL_SNR)
    cfg, B, K, W = LinkConfig(sim, m), _band(name, B), 3, 2 * R
    E = equal_estimates(est, R, K)
    assert np.array_equal(rho.reshape(-1, K, W), np.broadcast_to(rho.reshape(-1, K, W)[:, :1], (FRAMES // (K * W), K, W)))
    assert len(np.unique(rho)) > 1 and not np.array_equal(ideal.reshape(-1, K, W, *sim.ofdm)[:, 0], ideal.reshape(-1, K, W, *sim.ofdm)[:, 1])
    for d in (1, 2):
        sent, _ = delayed_groups(FRAMES // W, K, d)
        at = (sent[:, None] * W + np.arange(W)[None, :]).ravel()
        want = link_precoded_host(cfg, keys[at], ideal[at], E[at], sigma[at], rho[at], scale[sent], R, B, (1.0, 0.5))
        _same(link_precoded_host(cfg, keys, ideal, E, sigma, rho, scale, R, B, (1.0, 0.5), slots=K, delay=d), want)


@pytest.mark.parametrize("name,R,m,B", CASES)
def test_the_applied_pmi_is_the_selection_on_the_feedback_groups(name, R, m, B):
    sim, keys, sigma, ideal, est, rho, scale = delay_operands(name, R)
    cfg, B, W = LinkConfig(sim, m), _band(name, B), 2 * R
    every = precoding_pmi_host(cfg, est, rho, R, B)                              # the selection of every input group
    differ = 0
    for K, d in ((3, 1), (3, 2), (2, 1)) if R == 1 else ((3, 1), (3, 2)):
        sent, feedback = delayed_groups(FRAMES // W, K, d)
        out = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, slots=K, delay=d)
        assert out[3].dtype == np.int32 and np.array_equal(out[3], every[feedback])
        assert np.array_equal(precoding_pmi_host(cfg, est, rho, R, B, slots=K, delay=d), every[feedback])
        pmi, flags = precoding_pmi_host(cfg, est, rho, R, B, 1e-4, slots=K, delay=d)
        want_pmi, want_flags = precoding_pmi_host(cfg, est, rho, R, B, 1e-4)
        assert np.array_equal(pmi, want_pmi[feedback]) and np.array_equal(flags, want_flags[feedback])
        differ += int((every[feedback] != every[sent]).sum())
        # ... and the rest is the instantaneous link on the transmit groups with those PMIs forced
        at = (sent[:, None] * W + np.arange(W)[None, :]).ravel()
        _same(out, link_precoded_host(cfg, keys[at], ideal[at], est[at], sigma[at], rho[at], scale[sent], R, B, pmi=every[feedback]))
    if B == 1 and name == "odd_30x7":
        assert differ > 0                                       # stale PMIs do differ from the slots' own: the comparison is not vacuous


def test_the_feedback_groups_rho_is_what_the_selection_reads():
    """R = 2 with weights that differ between slots: swapping the feedback slot's rho changes the applied PMIs of some subband, the
    transmit slot's rho does not enter the selection."""
    name, R, B = "odd_30x7", 2, 1
    sim, keys, sigma, ideal, est, rho, scale = delay_operands(name, R)
    cfg = LinkConfig(sim, 4)
    base = precoding_pmi_host(cfg, est, rho, R, B, slots=3, delay=1)
    other = rho.copy().reshape(-1, 3, 4)
    other[:, 2] = np.float32(0.25) * other[:, 2]                                 # slot 2 is transmit-only at d = 1
    other[:, 2, 0] = 1
    assert np.array_equal(precoding_pmi_host(cfg, est, other.reshape(-1), R, B, slots=3, delay=1), base)
    other = rho.copy().reshape(-1, 3, 4)
    other[:, 0, 2] = np.float32(40.0)                                            # slot 0 feeds slot 1: antenna 1 outweighs antenna 0
    assert not np.array_equal(precoding_pmi_host(cfg, est, other.reshape(-1), R, B, slots=3, delay=1), base)


@pytest.mark.parametrize("K,d", [(3, 2), (2, 1)])
def test_compact_output_rows_index_by_index(K, d):
    name, R, m, B = "odd_30x7", 1, 4, 7
    sim, keys, sigma, ideal, est, rho, scale = delay_operands(name, R)
    cfg, W = LinkConfig(sim, m), 2
    G = FRAMES // W
    counts, loss, llr, pmi = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, (1.0, 0.5), slots=K, delay=d)
    Q = G // K
    assert counts.shape == (Q * (K - d), 2) and loss.shape == (Q * (K - d), 2) and llr.shape == (Q * (K - d), 30, 7, m)
    assert pmi.shape == (Q * (K - d), 5)
    seen = set()
    for seq in range(Q):
        for k in range(d, K):
            o, gt, gf = seq * (K - d) + (k - d), seq * K + k, seq * K + k - d
            seen.add(o)
            fb, tx = slice(gf * W, gf * W + W), slice(gt * W, gt * W + W)
            chosen = precoding_pmi_host(cfg, est[fb], rho[fb], R, B)
            one = link_precoded_host(cfg, keys[tx], ideal[tx], est[tx], sigma[tx], rho[tx], scale[gt:gt + 1], R, B, (1.0, 0.5), pmi=chosen)
            _same([counts[o:o + 1], loss[o:o + 1], llr[o:o + 1], pmi[o:o + 1]], one)
    assert seen == set(range(Q * (K - d)))


def test_refusals():
    name, R, B = "odd_30x7", 1, 7
    sim, keys, sigma, ideal, est, rho, scale = delay_operands(name, R)
    cfg = LinkConfig(sim, 4)
    args = (cfg, keys, ideal, est, sigma, rho, scale, R, B)
    for kw in (dict(slots=3, delay=3), dict(slots=3, delay=-1), dict(slots=0, delay=0), dict(slots=1, delay=1), dict(slots=5, delay=1),
               dict(slots=7, delay=0), dict(slots=2.0, delay=1), dict(slots=3, delay=True)):
        with pytest.raises(ValueError):
            link_precoded_host(*args, **kw)
        with pytest.raises(ValueError):
            precoding_pmi_host(cfg, est, rho, R, B, **kw)
    with pytest.raises(ValueError, match="scale must hold one value per group"):
        link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale[:8], R, B, slots=3, delay=1)
    with pytest.raises(ValueError, match="pmi must hold"):
        link_precoded_host(*args, slots=3, delay=1, pmi=np.zeros((12, 5), np.int32))         # the compact rows: 8
    link_precoded_host(*args, slots=3, delay=1, pmi=np.zeros((8, 5), np.int32))
    # the accumulators and the sweeps say what to use
    code, ldpc = CodeConfig(cfg, 64, "1/2"), LdpcConfig(LinkConfig(ChannelSimConfig(), 4), "1/2")
    for make in (lambda **kw: LinkAccumulator(cfg, "cpu", **kw), lambda **kw: RateAccumulator(cfg, "cpu", **kw),
                 lambda **kw: BlockErrorAccumulator(code, "cpu", **kw), lambda **kw: LdpcBlockErrorAccumulator(ldpc, "cpu", **kw)):
        with pytest.raises(ValueError, match="give precoding_subband= as well"):
            make(precoding_delay=1, slots=3)
        with pytest.raises(ValueError, match="give precoding_subband= as well"):
            make(precoding_delay=1, slots=3, tx_diversity="time")
        with pytest.raises(ValueError, match="use slots >= 3"):
            make(precoding_subband=7, precoding_delay=2, slots=2)
        with pytest.raises(ValueError, match="use slots >= 2"):
            make(precoding_subband=7, precoding_delay=1)
        for bad in (dict(precoding_delay=-1), dict(precoding_delay=1.0, slots=3), dict(slots=0), dict(precoding_delay=True, slots=3)):
            with pytest.raises(ValueError, match="precoding_delay"):
                make(precoding_subband=7, **bad)
        make(precoding_subband=7, slots=3)                                       # no delay: any slots
    with pytest.raises(TypeError, match="precoding_delay"):
        HarqAccumulator.__init__(object.__new__(HarqAccumulator), None, "cpu", precoding_delay=1)
    acc = LinkAccumulator(cfg, "cpu", SEED, precoding_subband=7, precoding_delay=1, slots=3)
    with pytest.raises(ValueError, match="not a multiple of slots \\* 2 \\* branches = 3 \\* 2 \\* 1"):
        acc.update(None, torch.from_numpy(ideal[:8].copy()), frame_ids=np.arange(8), snr_db=10.0)


def test_the_accumulators_and_the_sweeps_against_the_definition_batch_by_batch():
    """``precoding_delay=1, slots=3`` at 2 x 2 on the CPU, fed by the simulator's sequences: errors, losses, the histogram of the APPLIED
    PMIs and the decoders' counts are the definition's on each batch, with the leader keys of the transmit slots; ``frames`` counts the
    transmitted groups; the three sweeps of ``evaluation`` return the accumulators' results."""
    R, seed, B, K, d = 2, 5, 6, 3, 1
    sim = ChannelSimConfig(ofdm=(36, 14), pilot=(4, 2), slots=K, antennas=(R, 2), rx_correlation=0.4, snr_db=(6.0, 12.0),
                           doppler_hz=(1400.0,))
    link = LinkConfig(sim, 4)
    conv_code, ldpc_code = CodeConfig(link, 128, "1/2"), LdpcConfig(link, "1/2")
    loader = SynthLoader(sim, 24, 48, seed=seed)                                 # two sequences a batch, two batches
    kw = dict(seed=seed, branches=R, precoding_subband=B, precoding_delay=d, slots=K)
    hard, rate = LinkAccumulator(link, "cpu", **kw), RateAccumulator(link, "cpu", factors=(1.0, 0.5), **kw)
    conv, ldpc = BlockErrorAccumulator(conv_code, "cpu", **kw), LdpcBlockErrorAccumulator(ldpc_code, "cpu", **kw)
    instant = LinkAccumulator(link, "cpu", seed=seed, branches=R, precoding_subband=B, slots=K)
    want = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "pmi": np.zeros(4, np.int64), "conv": 0, "ldpc": 0}
    batches = 0
    for pilots, ideal, meta in loader:
        for acc in (hard, rate, conv, ldpc, instant):
            acc.update(None, ideal, meta)
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        H = ideal.numpy()
        out = link_precoded_host(link, keys, H, H, noise_sigma(snr), *precoding_weights(snr, 0.0, R), R, B, (1.0, 0.5), slots=K, delay=d)
        lead = np.ascontiguousarray(keys[::2 * R][delayed_groups(len(keys) // (2 * R), K, d)[0]])
        want["hard"] += out[0].sum(axis=0)
        want["loss"] += out[1].sum(axis=0)
        want["pmi"] += np.bincount(out[3].reshape(-1), minlength=4)
        llr = link_precoded_host(link, keys, H, H, noise_sigma(snr), *precoding_weights(snr, 0.0, R), R, B, slots=K, delay=d)[2]
        want["conv"] = want["conv"] + link_decode_host(conv_code, lead, llr)[0].sum(axis=0)
        want["ldpc"] = want["ldpc"] + link_ldpc_host(ldpc_code, lead, llr)[0].sum(axis=0)
        batches += 1
    groups = batches * 2 * (K - d)
    assert batches == 2 and all(a.frames == groups for a in (hard, rate, conv, ldpc)) and instant.frames == batches * 2 * K
    assert hard.errors.tolist() == want["hard"].tolist() and np.array_equal(rate.loss.numpy(), want["loss"])
    assert conv.errors.tolist() == want["conv"].tolist() and ldpc.errors.tolist() == want["ldpc"].tolist()
    for acc in (hard, rate, conv, ldpc):
        assert acc.pmi_histogram() == want["pmi"].tolist() and sum(acc.pmi_histogram()) == groups * 6
    assert hard.result() == want["hard"][0] / (groups * link.bits_per_frame)
    loaders = lambda: [("snr_1", SynthLoader(sim, 24, 48, seed=seed))]  # noqa: E731 -- a fresh loader per sweep: epoch 0 again
    common = dict(seed=seed, branches=R, precoding_subband=B, precoding_delay=d, slots=K)
    assert get_link_stats(None, loaders(), link, **common) == {1: hard.result()}
    assert get_link_rates(None, loaders(), link, factors=(1.0, 0.5), **common) == {1: rate.result_gmi()}
    assert get_link_bler(None, loaders(), conv_code, **common) == {1: conv.result()}
    assert get_link_bler(None, loaders(), ldpc_code, **common) == {1: ldpc.result()}
    print(f"2 x 2, d = {d}: BER {hard.result():.4f} against {instant.result():.4f} with instantaneous feedback; GMI {rate.result_gmi():.3f}")


# ---- what a stale precoder must show ----

def _stale(doppler_hz, delays, sequences=400, K=5):
    """{d: (share of subbands whose applied PMI differs from the transmit slot's own, bit errors on the slots d = max(delays) sends)} on
    the twins: 2 x 1, perfect channel knowledge, QPSK at 10 dB, slots of two symbols."""
    sim = ChannelSimConfig(ofdm=(24, 2), pilot=(4, 1), slots=K, antennas=(1, 2), snr_db=(10.0,), delay_spread_ns=(100.0,),
                           doppler_hz=(float(doppler_hz),))
    link = LinkConfig(sim, 2)
    n = sequences * K * 2
    ideal, _, meta = simulate_frames_host(sim, 7, np.arange(n))
    keys, snr = frame_keys(7, np.arange(n)), meta[:, 0]
    rho, scale = precoding_weights(snr, 0.0, 1)
    own = precoding_pmi_host(link, ideal, rho, 1, 4)                            # every slot's own selection
    last = max(delays)
    out = {}
    for d in delays:
        counts, _, _, pmi = link_precoded_host(link, keys, ideal, ideal, noise_sigma(snr), rho, scale, 1, 4, slots=K, delay=d)
        sent, _ = delayed_groups(n // 2, K, d)
        rows = np.flatnonzero(sent % K >= last)                                  # the slots every delay sends
        out[d] = (float((pmi != own[sent]).mean()), int(counts[rows, 0].sum()))
    return out


def test_a_still_channel_keeps_its_precoder():
    got = _stale(0.0, (0, 2), sequences=20)
    assert got[0][0] == 0.0 and got[2][0] == 0.0 and got[2][1] == got[0][1]


def test_a_stale_precoder_at_the_top_doppler_bin():
    got = _stale(1400.0, (0, 1, 4))
    print("1400 Hz, slots of 2 symbols: (stale share, bit errors on slot 4) at d = 0, 1, 4:", got)
    assert got[0][0] == 0.0 and got[1][0] >= 0.1 and got[4][0] >= got[1][0] + 0.1 and got[4][0] <= 0.85
    assert got[4][1] >= got[0][1] and got[0][1] > 0
