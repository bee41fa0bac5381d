"""``linksim``'s diversity link on the CPU: ``link_mrc_host`` against the single-branch definitions at R = 1, the two exact extremes,
a brute force over all ``2^m`` symbols, the weights (``branch_weights``) against the textbook ``1 / sigma_r^2`` combiner, the order of
the non-leader branches, the refusals, the four accumulators and the three sweeps of ``evaluation`` with ``branches=2`` against the
definition applied batch by batch, the binding, and the share of flagged decisions on the inputs tests/test_linkmrc_gpu.py compares
the kernel on.

``mrc_inputs`` builds those inputs once per grid; the GPU file imports it, so both files speak about the same arrays."""
import numpy as np
import pytest
import torch

from adafortitran_amd import _abi
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, simulate_frames_host
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, MAX_BRANCHES, BlockErrorAccumulator, CodeConfig, LdpcBlockErrorAccumulator,
                                      LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator, branch_weights, constellation,
                                      link_decode_host, link_errors_host, link_ldpc_host, link_llrs_host, link_mrc_host, llr_scale,
                                      noise_sigma)
from adafortitran_amd.lmmse import lmmse_estimate_host
from test_linksim import GRIDS, SEED, SHARE_CAP, TAU_CAP, flagged_share, link_inputs
from test_linksoft import sent_bits

MRC_GRIDS = {"default_120x14": 8, "odd_30x7": 16}           # frames [0, n) of seed 3: 1, 2, 4 and 8 branches divide both
BRANCHES = (1, 2, 4, 8)
MRC_ODD = "odd_last_alone_3x5"                              # its two frames: one group of two branches, or two of one
_inputs = {}


def mrc_inputs(name):
    """(sim, keys uint64 [n], sigma float32 [n], snr float64 [n], ideal complex64 [n,S,T], {"lmmse": .., "ideal": ..}), made once per
    grid and read-only: ``test_linksim.link_inputs``' recipe on more frames, each at the SNR it was drawn with."""
    if name not in _inputs:
        sim, n = GRIDS[name][0], MRC_GRIDS[name] if name in MRC_GRIDS else GRIDS[name][1]
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(n))
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        est = {"lmmse": lmmse_estimate_host(sim, pilots, meta).astype(np.complex64), "ideal": ideal}
        keys, sigma, snr = frame_keys(SEED, np.arange(n)), noise_sigma(meta[:, 0]), meta[:, 0].astype(np.float64)
        for a in (ideal, est["lmmse"], keys, sigma, snr):
            a.setflags(write=False)
        _inputs[name] = (sim, keys, sigma, snr, ideal, est)
    return _inputs[name]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_one_branch_is_the_single_branch_link_exactly(m):
    factors = (1.0, 0.5, 0.125)
    for name in ("default_120x14", "odd_30x7", "one_data_element_2x1", "no_data_element_1x1"):
        sim, keys, sigma, ideal, est = link_inputs(name)
        cfg, n = LinkConfig(sim, m), len(keys)
        scale = llr_scale(np.linspace(3.0, 21.0, n))
        rho = np.ones(n, dtype=np.float32)
        for which in est:
            got = link_mrc_host(cfg, keys, ideal, est[which], sigma, rho, scale, 1, factors, tau=TAU_CAP, e_lambda=TAU_CAP)
            hard = link_errors_host(cfg, keys, ideal, est[which], sigma, tau=TAU_CAP)
            soft = link_llrs_host(cfg, keys, ideal, est[which], sigma, scale, factors, e_lambda=TAU_CAP)
            want = (hard[0], soft[0], soft[1], hard[1], hard[2], soft[2], soft[3], soft[4])
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
            plain = link_mrc_host(cfg, keys, ideal, est[which], sigma, rho, scale, 1, factors)
            assert len(plain) == 3 and all(np.array_equal(g, w) for g, w in zip(plain, want[:3]))
            assert len(link_mrc_host(cfg, keys, ideal, est[which], sigma, rho, scale, 1, factors, tau=TAU_CAP)) == 5
            assert len(link_mrc_host(cfg, keys, ideal, est[which], sigma, rho, scale, 1, factors, e_lambda=TAU_CAP)) == 6


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
@pytest.mark.parametrize("R", (2, 4))
def test_the_two_exact_extremes(R, m):
    for name in MRC_GRIDS:
        sim, keys, sigma, snr, ideal, _ = mrc_inputs(name)
        cfg, G = LinkConfig(sim, m), len(keys) // R
        rho, scale = branch_weights(snr, 0.0, R)
        zero = np.zeros_like(sigma)
        counts, loss, llr, wrong, flags = link_mrc_host(cfg, keys, ideal, ideal, zero, rho, scale, R, tau=TAU_CAP)
        assert counts.shape == (G, 2) and counts.dtype == np.int64 and loss.shape == (G, 1) and llr.shape == (G, *sim.ofdm, m)
        assert not counts.any() and not wrong.any() and not flags.any()          # the estimates are the channels and there is no noise
        if m == 2:                                                               # the estimates point the other way: every bit flips
            counts, _, _, _, flags = link_mrc_host(cfg, keys, ideal, -ideal, zero, rho, scale, R, tau=TAU_CAP)
            assert (counts[:, 0] == 2 * cfg.data_elements).all() and (counts[:, 1] == cfg.data_elements).all() and not flags.any()
    if R == 2:                                     # the odd grid whose last element is data: the MSB of each axis flips at every m
        sim, keys, sigma, snr, ideal, _ = mrc_inputs(MRC_ODD)
        rho, scale = branch_weights(snr, 0.0, R)
        zero = np.zeros_like(sigma)
        assert not link_mrc_host(LinkConfig(sim, m), keys, ideal, ideal, zero, rho, scale, R)[0].any()
        assert link_mrc_host(LinkConfig(sim, m), keys, ideal, -ideal, zero, rho, scale, R)[0].tolist() == [[28, 14]]


def _received(cfg, keys, ideal, sigma, R):
    """x [G,S,T] of the leaders' words and y [n,S,T] of every branch, rebuilt from the documented streams: float64."""
    from adafortitran_amd.chansim import words
    (S, T), m = cfg.sim.ofdm, cfg.bits_per_symbol
    q = np.arange(S * T, dtype=np.uint64).reshape(1, S, T)
    w = (words(keys[::R, None, None], 5, q) >> np.uint64(64 - m)).astype(np.int64)
    x = constellation(m)[w]
    u1, u2 = (((words(keys[:, None, None], s, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23 for s in (6, 7))
    noise = sigma.astype(np.float64)[:, None, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)
    return x, ideal.astype(np.complex128) * np.repeat(x, R, axis=0) + noise


def _brute_force(cfg, y, E, weight, R):
    """[G,S,T,m]: min over the symbols with bit 1 minus min over those with bit 0 of ``sum_r weight_r |y_r - E_r x|^2``."""
    m, pts = cfg.bits_per_symbol, constellation(cfg.bits_per_symbol)
    dist = weight[:, None, None, None] * np.abs(y[..., None] - E.astype(np.complex128)[..., None] * pts) ** 2      # [n,S,T,2^m]
    dist = dist.reshape(-1, R, *dist.shape[1:])
    total = dist[:, 0]
    for r in range(1, R):
        total = total + dist[:, r]
    word = np.arange(1 << m)
    out = np.empty((*total.shape[:3], m))
    for j in range(m):
        one = ((word >> (m - 1 - j)) & 1).astype(bool)
        out[..., j] = total[..., one].min(axis=-1) - total[..., ~one].min(axis=-1)
    return out * cfg.data_mask[None, :, :, None]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_llrs_against_a_brute_force_over_all_symbols(m):
    """scale_leader sum_r rho_r |y_r - E_r x|^2 over all 2^m symbols: pins the separable form, the weights and the leader's scale."""
    R = 3
    sim, keys, sigma, snr, ideal, est = mrc_inputs("odd_30x7")
    keys, sigma, snr, ideal, e = keys[:15], sigma[:15], snr[:15], ideal[:15], est["lmmse"][:15]
    cfg = LinkConfig(sim, m)
    rho, scale = branch_weights(snr, 0.01, R)
    assert (rho != 1).any() and len(set(scale.tolist())) > 1
    _, _, llr, _, _, q = link_mrc_host(cfg, keys, ideal, e, sigma, rho, scale, R, e_lambda=TAU_CAP)
    _, y = _received(cfg, keys, ideal, sigma, R)
    weight = np.repeat(scale.astype(np.float64), R) * rho.astype(np.float64)
    want = _brute_force(cfg, y, e, weight, R)
    assert (np.abs(llr - want) <= 1e-9 * q).all() and (q[:, cfg.data_mask] > 0).all() and (q[:, ~cfg.data_mask] == 0).all()


def test_the_weights():
    snr = np.array([0.0, 25.0, 10.0, 10.0, 30.0, 5.0])
    for err_var in (0.0, 0.02):
        for R in (1, 2, 3, 6):
            rho, scale = branch_weights(snr, err_var, R)
            assert rho.dtype == scale.dtype == np.float32 and rho.shape == (6,) and scale.shape == (6 // R,)
            assert (rho[::R] == 1).all() and scale.tobytes() == llr_scale(snr, err_var)[::R].tobytes()
            s = llr_scale(snr, err_var).astype(np.float64).reshape(-1, R)
            assert rho.tobytes() == (s / s[:, :1]).astype(np.float32).tobytes()
    rho, scale = branch_weights(np.full(8, 17.0), 0.0, 4)
    assert (rho == 1).all() and scale.tolist() == [float(llr_scale(17.0))] * 2
    assert branch_weights(snr)[0].tolist() == [1.0] * 6


@pytest.mark.parametrize("m", (2, 6))
def test_mixed_snr_is_the_combiner_with_inverse_noise_variances(m):
    """The textbook combiner, ``sum_r |y_r - E_r x|^2 / sigma_r^2`` in float64 with ``sigma_r^2 = 10^(-snr_r / 10)``.  The definition
    differs from it by the float32 roundings of ``rho``, ``scale`` and (in the noise) ``sigma``: each within 2^-24, a few 1e-7 of a
    metric in all, and a metric is at most ``q`` in size -- hence 1e-6 of ``q``."""
    R = 4
    sim, keys, sigma, snr, ideal, est = mrc_inputs("odd_30x7")
    cfg = LinkConfig(sim, m)
    rho, scale = branch_weights(snr, 0.0, R)
    assert rho.max() > 10 and rho.min() < 0.5                                    # the SNRs are mixed
    _, _, llr, _, _, q = link_mrc_host(cfg, keys, ideal, est["lmmse"], sigma, rho, scale, R, e_lambda=TAU_CAP)
    _, y = _received(cfg, keys, ideal, sigma, R)
    want = _brute_force(cfg, y, est["lmmse"], 10.0 ** (snr / 10.0), R)
    assert (np.abs(llr - want) <= 1e-6 * q).all()


def test_permuting_the_non_leader_branches():
    R = 4
    sim, keys, sigma, snr, ideal, est = mrc_inputs("default_120x14")
    cfg = LinkConfig(sim, 4)
    rho, scale = branch_weights(snr, 0.0, R)
    order = np.array([0, 3, 1, 2, 4, 6, 7, 5])
    rho_p, scale_p = branch_weights(snr[order], 0.0, R)
    assert scale_p.tobytes() == scale.tobytes() and rho_p.tobytes() == rho[order].tobytes()
    a = link_mrc_host(cfg, keys, ideal, est["lmmse"], sigma, rho, scale, R, (1.0, 0.25))
    b = link_mrc_host(cfg, keys[order], ideal[order], est["lmmse"][order], sigma[order], rho_p, scale_p, R, (1.0, 0.25))
    assert np.array_equal(a[0], b[0]) and (np.abs(a[1] - b[1]) <= 1e-12 * a[1]).all()
    # ... while another leader is another transmission
    c = link_mrc_host(cfg, keys[::-1], ideal[::-1], est["lmmse"][::-1], sigma[::-1], *branch_weights(snr[::-1], 0.0, R), R)
    assert not np.array_equal(a[0], c[0][::-1])


def test_refusals():
    sim, keys, sigma, snr, ideal, est = mrc_inputs("odd_30x7")
    cfg = LinkConfig(sim, 4)
    rho, scale = branch_weights(snr, 0.0, 4)
    for bad in (0, 9, 2.0, -1, True, "2"):
        with pytest.raises(ValueError, match="branches"):
            link_mrc_host(cfg, keys, ideal, ideal, sigma, rho, scale, bad)
        with pytest.raises(ValueError, match="branches"):
            branch_weights(snr, 0.0, bad)
        with pytest.raises(ValueError, match="branches"):
            LinkAccumulator(cfg, "cpu", branches=bad)
    assert MAX_BRANCHES == 8
    with pytest.raises(ValueError, match="16 frames is not a multiple of branches = 3"):
        link_mrc_host(cfg, keys, ideal, ideal, sigma, rho, scale, 3)
    with pytest.raises(ValueError, match="not a multiple"):
        branch_weights(snr, 0.0, 5)
    with pytest.raises(ValueError, match="rho"):
        link_mrc_host(cfg, keys, ideal, ideal, sigma, rho[:8], scale, 4)
    for bad in (scale[:3], np.repeat(scale, 4)):
        with pytest.raises(ValueError, match="scale"):
            link_mrc_host(cfg, keys, ideal, ideal, sigma, rho, bad, 4)
    for make in (lambda: LinkAccumulator(cfg, "cpu", branches=4), lambda: RateAccumulator(cfg, "cpu", branches=4),
                 lambda: BlockErrorAccumulator(CodeConfig(cfg, 64), "cpu", branches=4)):
        with pytest.raises(ValueError, match="6 frames is not a multiple of branches = 4"):
            make().update(None, torch.from_numpy(ideal[:6].copy()), frame_ids=np.arange(6), snr_db=snr[:6])


class _Ls(torch.nn.Module):
    """The LS-interpolated estimate as a model ``evaluation.forward_pass`` can call."""

    def __init__(self, sim):
        super().__init__()
        self.sim = sim
        self.register_buffer("anchor", torch.zeros(1))

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.numpy()))


def test_accumulators_and_sweeps_with_two_branches_on_the_host():
    """A host ``SynthLoader`` (every frame at its own SNR), three batches of four frames: each accumulator and each sweep equals the
    definition applied batch by batch, the coded ones through the host decoders on the definition's LLRs rounded to float32."""
    from adafortitran_amd.evaluation import get_link_bler, get_link_rates, get_link_stats
    R, seed, err_var = 2, 5, 0.01
    sim = GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code, ldpc = CodeConfig(cfg, 64, "1/2"), LdpcConfig(cfg, (3, 6))
    factors = (1.0, 0.5)
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 4, 12, device="cpu", seed=seed))
    assert len(batches) == 3
    hard, rate = LinkAccumulator(cfg, "cpu", seed, branches=R), RateAccumulator(cfg, "cpu", seed, factors, err_var, branches=R)
    conv, lay = BlockErrorAccumulator(code, "cpu", seed, err_var, branches=R), LdpcBlockErrorAccumulator(ldpc, "cpu", seed, err_var, R)
    want = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "loss0": np.zeros(8), "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64),
            "conv0": np.zeros(2, np.int64)}
    for pilots, ideal, meta in batches:
        est = model(pilots)
        for acc in (hard, rate, conv, lay):
            acc.update(est, ideal, meta)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        snr = meta[1].numpy().reshape(-1)
        for ev, tag in ((0.0, "0"), (err_var, "")):
            rho, scale = branch_weights(snr, ev, R)
            counts, loss, llr = link_mrc_host(cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), rho, scale, R,
                                              factors if tag == "" else np.asarray([2.0 ** -k for k in range(8)]))
            if tag == "0":
                want["hard"] += counts.sum(axis=0)
                want["loss0"] += loss.sum(axis=0)
                want["conv0"] += link_decode_host(code, keys[::R], llr.astype(np.float32))[0].sum(axis=0)
            else:
                want["loss"] += loss.sum(axis=0)
                want["conv"] += link_decode_host(code, keys[::R], llr.astype(np.float32))[0].sum(axis=0)
                want["ldpc"] += link_ldpc_host(ldpc, keys[::R], llr.astype(np.float32))[0].sum(axis=0)
    G = 6                                                                        # frames counts groups: per transmission
    assert hard.frames == rate.frames == conv.frames == lay.frames == G
    assert hard.errors.tolist() == want["hard"].tolist() and hard.result() == want["hard"][0] / (G * cfg.bits_per_frame)
    assert hard.result_ser() == want["hard"][1] / (G * cfg.data_elements)
    assert np.array_equal(rate.loss.numpy(), want["loss"])
    assert rate.result() == [4 - v / (G * cfg.data_elements) for v in want["loss"]]
    assert conv.errors.tolist() == want["conv"].tolist() and conv.result() == want["conv"][1] / (G * code.blocks)
    assert lay.errors.tolist() == want["ldpc"].tolist() and lay.result() == want["ldpc"][1] / (G * ldpc.blocks)
    assert lay.result_throughput() == (G * ldpc.blocks - want["ldpc"][1]) * ldpc.info_bits / (G * cfg.data_elements)
    # the sweeps (err_var 0 unless given), over a loader that replays the same frames
    loaders = [("SNR_0", SynthLoader(sim, 4, 12, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_stats(model, loaders, cfg, seed, branches=R) == {0: want["hard"][0] / (G * cfg.bits_per_frame)}
    assert get_link_rates(model, loaders, cfg, seed, branches=R) == {0: max(4 - v / (G * cfg.data_elements) for v in want["loss0"])}
    assert get_link_bler(model, loaders, code, seed, branches=R) == {0: want["conv0"][1] / (G * code.blocks)}
    assert get_link_bler(model, loaders, ldpc, seed, err_var, branches=R) == {0: want["ldpc"][1] / (G * ldpc.blocks)}
    # one branch over the same frames: the four accumulators against the single-branch definitions called directly
    hard1, rate1 = LinkAccumulator(cfg, "cpu", seed), RateAccumulator(cfg, "cpu", seed, factors, err_var)
    conv1, lay1 = BlockErrorAccumulator(code, "cpu", seed, err_var), LdpcBlockErrorAccumulator(ldpc, "cpu", seed, err_var)
    want1 = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64)}
    for pilots, ideal, meta in batches:
        est = model(pilots)
        for acc in (hard1, rate1, conv1, lay1):
            acc.update(est, ideal, meta)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        snr = meta[1].numpy().reshape(-1)
        want1["hard"] += link_errors_host(cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr)).sum(axis=0)
        loss, llr = link_llrs_host(cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), llr_scale(snr, err_var), factors)
        want1["loss"] += loss.sum(axis=0)
        want1["conv"] += link_decode_host(code, keys, llr.astype(np.float32))[0].sum(axis=0)
        want1["ldpc"] += link_ldpc_host(ldpc, keys, llr.astype(np.float32))[0].sum(axis=0)
    assert all(acc.branches == 1 and acc.frames == 12 for acc in (hard1, rate1, conv1, lay1))
    assert hard1.errors.tolist() == want1["hard"].tolist() and hard1.result() == want1["hard"][0] / (12 * cfg.bits_per_frame)
    np.testing.assert_allclose(rate1.loss.numpy(), want1["loss"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rate1.result(), [4 - v / (12 * cfg.data_elements) for v in want1["loss"]], rtol=1e-12, atol=0)
    assert conv1.errors.tolist() == want1["conv"].tolist() and conv1.result() == want1["conv"][1] / (12 * code.blocks)
    assert lay1.errors.tolist() == want1["ldpc"].tolist() and lay1.result() == want1["ldpc"][1] / (12 * ldpc.blocks)
    assert lay1.result_iterations() == want1["ldpc"][2] / (12 * ldpc.blocks)
    assert want1["hard"][0] > want["hard"][0] > 0                                # the frames are not trivial: diversity removed errors


def test_diversity_removes_errors():
    """The issue's prototype: seed 3, default grid, frames 0..7, LMMSE estimate, 16-QAM."""
    sim, keys, sigma, snr, ideal, est = mrc_inputs("default_120x14")
    cfg = LinkConfig(sim, 4)
    errors = {}
    for R in (1, 2, 4):
        rho, scale = branch_weights(snr, 0.0, R)
        errors[R] = (int(link_mrc_host(cfg, keys, ideal, est["lmmse"], sigma, rho, scale, R)[0][:, 0].sum()), cfg.bits_per_frame * 8 // R)
    assert errors == {1: (12301, 52992), 2: (4262, 26496), 4: (1351, 13248)}
    assert errors[1][0] == int(link_errors_host(cfg, keys, ideal, est["lmmse"], sigma)[:, 0].sum())


def test_the_sent_word_is_the_leaders():
    sim, keys, sigma, snr, ideal, _ = mrc_inputs("odd_30x7")
    cfg = LinkConfig(sim, 6)
    rho, scale = branch_weights(snr, 0.0, 4)
    _, _, llr = link_mrc_host(cfg, keys, ideal, ideal, np.zeros_like(sigma), rho, scale, 4)
    sent = sent_bits(cfg, keys[::4])
    assert ((llr < 0) == (sent == 1))[:, cfg.data_mask].all()                     # noiseless, perfect knowledge: the sign is the sent bit


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    import ctypes as C
    assert _abi.AFT_ABI_VERSION == 10 and _abi.AFT_LINK_MAX_BRANCHES == 8
    restype, argtypes = _abi.SIGNATURES["aft_link_mrc_f32"]
    assert "aft_link_mrc_f32" in _abi.EXPORTED_SYMBOLS and restype is C.c_int and len(argtypes) == 15
    assert argtypes[0]._type_ is _abi.AftLink and [i for i, t in enumerate(argtypes) if t is C.c_int] == [8, 9, 13]
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_mrc_f32") == names.index("aft_link_ldpc_f32") + 1                 # the header's order


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_flagged_share_on_the_inputs_the_gpu_tests_use(m):
    worst, weight = 0.0, 0.0
    for name in MRC_GRIDS:
        sim, keys, sigma, snr, ideal, est = mrc_inputs(name)
        cfg = LinkConfig(sim, m)
        for R in BRANCHES:
            rho, scale = branch_weights(snr, 0.0, R)
            weight = max(weight, float(rho.max()))
            for which in est:
                flags = link_mrc_host(cfg, keys, ideal, est[which], sigma, rho, scale, R, tau=TAU_CAP)[4]
                share = flagged_share(cfg, flags)
                assert share <= SHARE_CAP, (name, R, which, share)
                worst = max(worst, share)
    print(f"m = {m}: the largest flagged share at tau = {TAU_CAP} is {worst:.2e}; rho reaches {weight:.0f}")
