"""``adafortitran_amd.linksim``'s soft half on the CPU: the definition of the max-log LLRs and of the loss the achievable rate is read
from (their sign against the hard receiver, the exact extremes, pilots, the factors, the interval, the QPSK closed form, the orderings
that must hold), how wide the interval is on the inputs tests/test_linksoft_gpu.py compares the kernel on, ``RateAccumulator`` /
``get_link_rates`` on the host and over two gloo ranks, the new entry point in the signature table.

``soft_inputs`` adds the LLR scale to ``test_linksim.link_inputs``; the GPU file imports it, so both files speak about the same arrays."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from adafortitran_amd import _abi, ingest
from adafortitran_amd.chansim import (STREAM_DATA_BITS, ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, make_pack,
                                      simulate_frames_host, words)
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DEFAULT_FACTORS, LinkConfig, RateAccumulator, link_errors_host, link_llrs_host,
                                      llr_scale, noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator, lmmse_estimate_host
from test_linksim import GRIDS, SEED, SHARE_CAP, TAU_CAP, _free_port, link_inputs  # noqa: F401  (SHARE_CAP: re-exported to the GPU file)

WIDTH_CAP = 2e-2               # the issue's: the interval at e_lambda = TAU_CAP is at most this share of the loss it encloses


def soft_inputs(name):
    """``link_inputs(name)`` and the frames' LLR scale, float32 ``[n]``: one over the noise variance, ``1 / sigma^2`` formed in double."""
    sim, keys, sigma, ideal, est = link_inputs(name)
    scale = (1.0 / sigma.astype(np.float64) ** 2).astype(np.float32)
    scale.setflags(write=False)
    return sim, keys, sigma, scale, ideal, est


def sent_bits(cfg, keys):
    """int64 ``[n, S, T, m]``: the bits of every element's sent word, MSB first (I-axis bits, then Q-axis bits)."""
    (S, T), m = cfg.sim.ofdm, cfg.bits_per_symbol
    w = (words(np.asarray(keys)[:, None, None], STREAM_DATA_BITS, np.arange(S * T, dtype=np.uint64).reshape(1, S, T))
         >> np.uint64(64 - m)).astype(np.int64)
    return (w[..., None] >> np.arange(m - 1, -1, -1)) & 1


def test_llr_scale_and_the_default_factors():
    assert DEFAULT_FACTORS == (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125)
    s = llr_scale([0.0, 10.0, 30.0])
    assert s.dtype == np.float32 and s.tolist() == [1.0, np.float32(1.0 / 10.0 ** -1.0), np.float32(1.0 / 10.0 ** -3.0)]
    assert llr_scale(10.0, 0.1) == np.float32(1.0 / (0.1 + 0.1)) and llr_scale(np.float32(7.3)).shape == ()
    sim, keys, sigma, scale, ideal, _ = soft_inputs("one_data_element_2x1")
    cfg = LinkConfig(sim, 2)
    for bad in ((), np.ones(9)):
        with pytest.raises(ValueError, match="factors"):
            link_llrs_host(cfg, keys, ideal, ideal, sigma, scale, bad)
    with pytest.raises(ValueError, match="scale must hold one value per frame"):
        link_llrs_host(cfg, keys, ideal, ideal, sigma, np.ones(3))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_sign_of_the_llrs_is_the_hard_receivers_decision(m):
    """The nearest level carries the smallest metric, so the bits ``Lambda < 0`` are the hard demapper's: they differ from the sent
    bits where ``link_errors_host`` counts a wrong bit, except where a decision is within ``TAU_CAP`` of a boundary."""
    for snr in (0.0, 10.0, 20.0, 30.0):
        sim = ChannelSimConfig(snr_db=(snr,))
        cfg = LinkConfig(sim, m)
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(2))
        ideal = ideal.astype(np.complex64)
        keys, sigma = frame_keys(SEED, np.arange(2)), noise_sigma(meta[:, 0])
        sent = sent_bits(cfg, keys)
        for est in (ideal, ls_interpolate(sim, pilots.astype(np.complex64))):
            _, wrong, flags = link_errors_host(cfg, keys, ideal, est, sigma, tau=TAU_CAP)
            loss, llr = link_llrs_host(cfg, keys, ideal, est, sigma, llr_scale(meta[:, 0]))
            soft = (((llr < 0) ^ (sent == 1)) & cfg.data_mask[None, :, :, None])
            half = m // 2
            per_axis = np.stack([soft[..., :half].sum(axis=-1), soft[..., half:].sum(axis=-1)], axis=-1)
            differ = soft.sum(axis=-1) != wrong
            assert not (differ & ~flags.any(axis=-1)).any()
            assert wrong.sum() > 0 or snr >= 20.0
            assert (per_axis <= half).all() and loss.shape == (2, 1) and (loss >= 0).all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_exact_extremes(m):
    for name in GRIDS:
        sim, keys, sigma, scale, ideal, _ = soft_inputs(name)
        cfg = LinkConfig(sim, m)
        n = len(keys)
        # an estimate of zero says nothing: every LLR is exactly 0 and every bit costs one bit, at every factor
        loss, llr = link_llrs_host(cfg, keys, ideal, np.zeros_like(ideal), sigma, scale, DEFAULT_FACTORS)
        assert llr.shape == (n, *sim.ofdm, m) and loss.shape == (n, 8) and not llr.any()
        np.testing.assert_allclose(loss, m * cfg.data_elements, rtol=1e-13, atol=0)
        # ... and so does a factor of zero, whatever the estimate
        loss, llr = link_llrs_host(cfg, keys, ideal, ideal, sigma, scale, (0.0, 1.0))
        np.testing.assert_allclose(loss[:, 0], m * cfg.data_elements, rtol=1e-13, atol=0)
        assert (loss[:, 1] <= loss[:, 0]).all()
        # the estimate is the channel and there is no noise: no LLR points away from its sent bit
        loss, llr = link_llrs_host(cfg, keys, ideal, ideal, np.zeros_like(sigma), scale)
        sent = sent_bits(cfg, keys)
        mask = cfg.data_mask[None, :, :, None]
        assert (((llr < 0) == (sent == 1)) | ~mask).all() and ((llr != 0) | ~mask).all()
        assert (loss <= m * cfg.data_elements).all()                             # no bit costs more than the one it carries
        if cfg.data_elements == 0:
            assert not loss.any() and not llr.any()


def test_pilot_positions_carry_llr_zero():
    sim = ChannelSimConfig(pilot=(4, 3), pilot_scs=(0, 7, 118, 119), pilot_symbols=(0, 1, 13))
    cfg = LinkConfig(sim, 6)
    ideal, _, meta = simulate_frames_host(sim, SEED, np.arange(2))
    keys, sigma = frame_keys(SEED, np.arange(2)), noise_sigma(meta[:, 0])
    loss, llr, lo, hi, q = link_llrs_host(cfg, keys, ideal, ideal, sigma, llr_scale(meta[:, 0]), e_lambda=TAU_CAP)
    pilot = np.zeros((120, 14), dtype=bool)
    pilot[np.ix_((0, 7, 118, 119), (0, 1, 13))] = True
    assert pilot.sum() == 12 and (cfg.data_mask == ~pilot).all()
    assert not llr[:, pilot].any() and not q[:, pilot].any()
    assert (llr[:, ~pilot] != 0).all() and (q[:, ~pilot] > 0).all()
    # ... and cost nothing: the loss is that of the data elements
    dense = LinkConfig(ChannelSimConfig(pilot=(1, 1), pilot_scs=(0,), pilot_symbols=(0,)), 6)
    loss_dense, llr_dense = link_llrs_host(dense, keys, ideal, ideal, sigma, llr_scale(meta[:, 0]))
    assert (llr_dense[:, ~pilot] == llr[:, ~pilot]).all()
    z = np.where(sent_bits(cfg, keys) == 1, llr_dense, -llr_dense)[:, ~pilot]
    np.testing.assert_allclose(loss[:, 0], np.logaddexp(0.0, z).sum(axis=(1, 2)) / np.log(2.0), rtol=1e-12)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_interval_encloses_the_loss(m):
    for name in GRIDS:
        sim, keys, sigma, scale, ideal, est = soft_inputs(name)
        cfg = LinkConfig(sim, m)
        for e in est.values():
            loss, llr, lo, hi, q = link_llrs_host(cfg, keys, ideal, e, sigma, scale, DEFAULT_FACTORS, e_lambda=TAU_CAP)
            assert (0 <= lo).all() and (lo <= loss).all() and (loss <= hi).all() and (q >= 0).all()
            wide = link_llrs_host(cfg, keys, ideal, e, sigma, scale, DEFAULT_FACTORS, e_lambda=10 * TAU_CAP)
            assert (wide[2] <= lo).all() and (hi <= wide[3]).all() and (wide[4] == q).all() and (wide[0] == loss).all()
            again = link_llrs_host(cfg, keys, ideal, e, sigma, scale, DEFAULT_FACTORS)
            assert (again[0] == loss).all() and (again[1] == llr).all()


def _awgn_bit_loss(mean):
    """(mean, variance) of ``log2(1 + exp(-L))`` for ``L ~ N(mean, 2 mean)``, the LLR of a sent bit on a BPSK-AWGN channel, by
    Gauss-Hermite quadrature: 1 - J and the per-bit variance the standard error is taken from."""
    t, w = np.polynomial.hermite.hermgauss(200)
    L = mean[..., None] + np.sqrt(2.0 * mean[..., None]) * np.sqrt(2.0) * t
    f = np.logaddexp(0.0, -L) / np.log(2.0)
    first = (f * w).sum(axis=-1) / np.sqrt(np.pi)
    return first, (f * f * w).sum(axis=-1) / np.sqrt(np.pi) - first ** 2


def test_qpsk_with_perfect_knowledge_follows_the_bpsk_awgn_capacity():
    """Max-log is exact at m = 2: with the channel known and scale = 1 / sigma^2, Lambda = -4 d comp / sigma^2 is the true LLR of its
    bit, Gaussian with mean 2 |H|^2 / sigma^2 and twice that variance given the channel.  The loss of a frame set is then a sum of
    independent terms whose means and variances the quadrature gives on the realised |H|^2: within 5 standard errors."""
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 2)
    ideal, _, meta = simulate_frames_host(sim, SEED, np.arange(8))
    keys, sigma = frame_keys(SEED, np.arange(8)), noise_sigma(meta[:, 0])
    loss, _ = link_llrs_host(cfg, keys, ideal, ideal, sigma, llr_scale(meta[:, 0]))
    mean = 2.0 * np.abs(ideal) ** 2 / sigma.astype(np.float64)[:, None, None] ** 2
    first, var = _awgn_bit_loss(mean)
    want = 2.0 * (first * cfg.data_mask).sum()
    se = np.sqrt(2.0 * (var * cfg.data_mask).sum())
    print(f"loss {loss.sum():.2f}  closed form {want:.2f}  standard error {se:.2f}")
    assert se > 0 and abs(loss.sum() - want) <= 5.0 * se


def test_the_orderings_that_must_hold():
    """Perfect knowledge at its best factor is worth at least the LMMSE estimate at its best factor, and more SNR is worth more."""
    m = 6
    best = {}
    for snr in (0.0, 10.0, 20.0):
        sim = ChannelSimConfig(snr_db=(snr,))
        cfg = LinkConfig(sim, m)
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(6))
        keys, sigma, scale = frame_keys(SEED, np.arange(6)), noise_sigma(meta[:, 0]), llr_scale(meta[:, 0])
        for which, e in (("perfect", ideal), ("lmmse", lmmse_estimate_host(sim, pilots, meta))):
            loss = link_llrs_host(cfg, keys, ideal, e, sigma, scale, DEFAULT_FACTORS)[0].sum(axis=0)
            best[which, snr] = float((m - loss / (6 * cfg.data_elements)).max())
    print({k: round(v, 3) for k, v in best.items()})
    assert all(best["perfect", snr] >= best["lmmse", snr] for snr in (0.0, 10.0, 20.0))
    assert 0 < best["perfect", 0.0] < best["perfect", 10.0] < best["perfect", 20.0] <= m


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_interval_is_narrow_on_the_inputs_the_gpu_tests_use(m):
    """tests/test_linksoft_gpu.py lets the kernel's loss fall anywhere in the interval, which says something only while the interval is
    narrow: at e_lambda = TAU_CAP its width is at most 2e-2 of the loss, summed over the frames of every input set used there."""
    worst = 0.0

    def width(cfg, keys, ideal, e, sigma, scale):
        loss, _, lo, hi, _ = link_llrs_host(cfg, keys, ideal, e, sigma, scale, DEFAULT_FACTORS, e_lambda=TAU_CAP)
        return (hi - lo).sum(axis=0), loss.sum(axis=0)

    totals = {}
    for name in GRIDS:
        sim, keys, sigma, scale, ideal, est = soft_inputs(name)
        for which, e in est.items():
            w, l = width(LinkConfig(sim, m), keys, ideal, e, sigma, scale)
            totals[which] = totals.get(which, 0) + np.stack([w, l])
    for which, (w, l) in totals.items():
        share = w / l
        worst = max(worst, float(share.max()))
        assert (share <= WIDTH_CAP).all(), (which, share)
    # the accumulator's sweep there: five batches of 16 from SynthLoader, seed 2 (the host twin of the device's frames)
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, m)
    total = 0
    for pil, ideal, meta in SynthLoader(sim, 16, 80, device="cpu", seed=2):
        g = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
        snr = meta[1].numpy().reshape(-1)
        total = total + np.stack(width(cfg, frame_keys(2, g), ideal.numpy(), ideal.numpy(), noise_sigma(snr), llr_scale(snr)))
    share = total[0] / total[1]
    worst = max(worst, float(share.max()))
    assert (share <= WIDTH_CAP).all(), share
    print(f"m = {m}: widest interval at e_lambda = {TAU_CAP:g}: {worst:.2e} of the loss")


def _loaders(sim):
    packs = {snr: make_pack(sim, 32, seed=20 + snr, snr_db=snr) for snr in (0, 20)}
    return packs, [(f"SNR_{snr}", ingest.ResidentLoader(p, sim.pilot, 16, device="cpu", shuffle=False)) for snr, p in packs.items()]


def test_rate_accumulator_and_sweep_on_the_cpu_over_two_loaders():
    from adafortitran_amd.evaluation import get_link_rates
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    packs, loaders = _loaders(sim)
    model = LmmseEstimator(sim)
    perfect, lmmse = get_link_rates(None, loaders, cfg, seed=5), get_link_rates(model, loaders, cfg, seed=5)
    one = get_link_rates(None, loaders, cfg, seed=5, factors=(1.0,))
    assert list(perfect) == list(lmmse) == list(one) == [0, 20]
    sc, sym = np.asarray(sim.pilot_scs), np.asarray(sim.pilot_symbols)
    for snr, pack in packs.items():
        keys, sigma, scale = frame_keys(5, np.arange(32)), noise_sigma(pack["meta"][:, 1]), llr_scale(pack["meta"][:, 1])
        est = lmmse_estimate_host(sim, pack["h_ls_sparse"][:, sc[:, None], sym[None, :]], pack["meta"][:, 1:4]).astype(np.complex64)
        for got, e in ((perfect[snr], pack["h_ideal"]), (lmmse[snr], est)):
            loss = sum(link_llrs_host(cfg, keys[i:i + 16], pack["h_ideal"][i:i + 16], e[i:i + 16], sigma[i:i + 16], scale[i:i + 16],
                                      DEFAULT_FACTORS)[0].sum(axis=0) for i in (0, 16))
            assert got == max(4 - v / (32 * cfg.data_elements) for v in loss.tolist())
        assert lmmse[snr] <= perfect[snr] and one[snr] <= perfect[snr]
    assert 0 < perfect[0] < perfect[20] <= 4
    # the accumulator by hand: explicit frame numbers and one SNR for the batch, an error variance, an empty sweep
    acc = RateAccumulator(cfg, "cpu", seed=5, factors=(1.0, 0.5), err_var=0.25)
    ideal = torch.from_numpy(packs[0]["h_ideal"])
    acc.update(None, ideal[:10], frame_ids=np.arange(10), snr_db=0.0)
    acc.update(ideal[10:], ideal[10:], frame_ids=torch.arange(10, 32), snr_db=torch.zeros(22))
    loss = link_llrs_host(cfg, frame_keys(5, np.arange(32)), packs[0]["h_ideal"], packs[0]["h_ideal"], noise_sigma(np.zeros(32)),
                          llr_scale(np.zeros(32), 0.25), (1.0, 0.5))[0]
    assert llr_scale(0.0, 0.25) == np.float32(0.8) and acc.frames == 32 and acc.loss.dtype == torch.float64
    np.testing.assert_allclose(acc.result(), 4 - loss.sum(axis=0) / (32 * cfg.data_elements), rtol=1e-12)
    assert acc.result_gmi() == max(acc.result()) and len(acc.result()) == 2
    assert RateAccumulator(cfg, "cpu").result() == [0.0] and RateAccumulator(cfg, "cpu").result_gmi() == 0.0
    with pytest.raises(ValueError, match="frame numbers"):
        acc.update(None, ideal[:2])
    with pytest.raises(ValueError, match="SNR"):
        acc.update(None, ideal[:2], frame_ids=[0, 1])
    with pytest.raises(ValueError, match="factors"):
        RateAccumulator(cfg, "cpu", factors=np.ones(9))
    with pytest.raises(ValueError, match="err_var"):
        RateAccumulator(cfg, "cpu", err_var=-1.0)
    with pytest.raises(ValueError, match="LinkConfig"):
        RateAccumulator(sim, "cpu")


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    sim = ChannelSimConfig(snr_db=(10.0,))
    acc = RateAccumulator(LinkConfig(sim, 4), "cpu", seed=SEED, factors=DEFAULT_FACTORS)
    for _, ideal, meta in SynthLoader(sim, 8, 24, device="cpu", seed=SEED, rank=rank, world_size=world, fresh_each_epoch=False):
        acc.update(None, ideal, meta)
    ret[rank] = (acc.result(), acc.result_gmi(), acc.frames)
    dist.destroy_process_group()


def test_two_gloo_ranks_report_the_same_rates():
    world = 2
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
        results = dict(ret)
    assert results[0][:2] == results[1][:2] and results[0][2] + results[1][2] == 24       # one gather, one sum: the same bits
    sim = ChannelSimConfig(snr_db=(10.0,))
    cfg = LinkConfig(sim, 4)
    ideal = simulate_frames_host(sim, SEED, np.arange(24))[0].astype(np.complex64)
    snr = np.full(24, 10.0)
    loss = link_llrs_host(cfg, frame_keys(SEED, np.arange(24)), ideal, ideal, noise_sigma(snr), llr_scale(snr), DEFAULT_FACTORS)[0]
    want = 4 - loss.sum(axis=0) / (24 * cfg.data_elements)
    np.testing.assert_allclose(results[0][0], want, rtol=1e-12)
    assert len(results[0][0]) == 8 and results[0][1] == max(results[0][0])


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    assert _abi.AFT_ABI_VERSION == 10 and "aft_link_soft_f32" in _abi.SIGNATURES and "aft_link_soft_f32" in _abi.EXPORTED_SYMBOLS
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_soft_f32") == names.index("aft_link_errors_f32") + 1       # the header's order
    restype, argtypes = _abi.SIGNATURES["aft_link_soft_f32"]
    assert len(argtypes) == 12 and argtypes[0]._type_ is _abi.AftLink
