"""Decision-directed refinement on the CPU, no library needed: the observation's definition (``linksim.link_observe_host``), the
orderings genie < one pass < initial at 20 dB, its decisions against the diversity link's, the ``decisions=`` round trip,
``DataAidedRefiner`` and the ``refine=`` keyword of the sweeps against the twins applied by hand, and the refusals.

The ordering test runs on 64 simulated frames; the figures it orders were measured on the twins before it was written (the docstring of
the test records them), and every step between them is above 19 % of the larger number."""
import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, ingest
from adafortitran_amd.chansim import ChannelSimConfig, frame_keys, ls_interpolate, make_pack, simulate_frames_host
from adafortitran_amd.evaluation import get_link_bler, get_link_harq, get_link_rates, get_link_stats, get_refined_test_stats, get_test_stats
from adafortitran_amd.linksim import (PILOT_DECISION, DataAidedRefiner, LdpcConfig, LinkAccumulator, LinkConfig, as_refiner, branch_weights,
                                      data_noise_scale, gray_level, link_mrc_host, link_observe_host, noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator, LmmseTables, lmmse_estimate_host, lmmse_grid_host

SEED = 5
_cache = {}

# grid and frames of the device tests (tests/test_linkdd_gpu.py, tests/test_lmmse_grid_gpu.py): tests/test_linksim.py's three grids and
# one with more subcarriers than a workgroup has threads; the frame counts let 1, 2 and 4 branches divide a batch
DD_GRIDS = {
    "default_120x14": (ChannelSimConfig(), 16),                                  # 16-byte accesses, 840 pairs over 256 threads, Kf = 12
    "odd_30x7": (ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3)), 8),              # odd T: the 8-byte paths, a ragged last pass
    "odd_last_alone_3x5": (ChannelSimConfig(ofdm=(3, 5), pilot=(1, 1)), 4),      # Kf = 3 < taps; element 14 is data, alone in its pair
    "tall_300x4": (ChannelSimConfig(ofdm=(300, 4), pilot=(6, 2)), 2),            # more subcarriers than threads: ten chunks of rows
}
_dd = {}


def dd_inputs(name):
    """(sim, keys uint64 [n], sigma float32 [n], snr [n], ideal, pilots, meta float32 [n, 3], est = the LMMSE estimate; all complex64),
    made once per grid and read-only: frames [0, n) of seed 3 from the float64 simulator, each at the SNR it was drawn with."""
    if name not in _dd:
        sim, n = DD_GRIDS[name]
        ideal, pilots, meta = simulate_frames_host(sim, 3, np.arange(n))
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        est = lmmse_estimate_host(sim, pilots, meta).astype(np.complex64)
        out = (sim, frame_keys(3, np.arange(n)), noise_sigma(meta[:, 0]), meta[:, 0].copy(), ideal, pilots, meta, est)
        for a in out[1:]:
            a.setflags(write=False)
        _dd[name] = out
    return _dd[name]


def _frames(snr_db, n=64):
    """(sim, tables, ideal, pilots, meta, keys, sigma) of frames [0, n) of seed 5 at one SNR, every other condition drawn; once."""
    if (snr_db, n) not in _cache:
        sim = ChannelSimConfig(snr_db=(float(snr_db),))
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(n))
        out = (sim, LmmseTables(sim), ideal, pilots, meta, frame_keys(SEED, np.arange(n)), noise_sigma(meta[:, 0]))
        for a in out[2:]:
            a.setflags(write=False)
        _cache[snr_db, n] = out
    return _cache[snr_db, n]


def _nmse(est, ideal):
    return float((np.abs(est - ideal) ** 2).mean() / (np.abs(ideal) ** 2).mean())


def _passes(snr_db, m, which, passes=1):
    """[initial NMSE, after one pass, ...] and the genie bound, by the twins alone."""
    sim, tb, ideal, pilots, meta, keys, sigma = _frames(snr_db)
    cfg, beta, rho = LinkConfig(sim, m), data_noise_scale(m), np.ones(len(keys), dtype=np.float32)
    e0 = (lmmse_estimate_host(tb, pilots, meta) if which == "lmmse" else ls_interpolate(sim, pilots)).astype(np.complex64)
    est, out = e0, [_nmse(e0, ideal)]
    for _ in range(passes):
        z, _, _ = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots)
        est = lmmse_grid_host(tb, z, meta, noise_scale=beta).astype(np.complex64)
        out.append(_nmse(est, ideal))
    z, _, _ = link_observe_host(cfg, keys, ideal, e0, sigma, rho, pilots, source="sent")
    return out, _nmse(lmmse_grid_host(tb, z, meta, noise_scale=beta), ideal)


@pytest.mark.parametrize("m", (2, 4))
@pytest.mark.parametrize("which", ("lmmse", "ls"))
def test_at_20_db_genie_beats_one_pass_beats_the_initial_estimate(which, m):
    """Measured on these 64 frames: LMMSE 0.206 -> 0.147 (QPSK) / 0.166 (16-QAM), LS 0.273 -> 0.188 / 0.214, genie 1.1e-4 / 2.1e-4:
    every step is at least 19 % of the larger number.  At 0 dB refinement HURTS the LMMSE estimate (0.306 -> 0.390 / 0.366: about
    half the decisions are wrong and each wrong one is a large error); those figures are printed, not asserted."""
    (initial, once), genie = _passes(20, m, which)
    print(f"20 dB m = {m} {which}: initial {initial:.4f}  one pass {once:.4f}  genie {genie:.3e}")
    assert genie < once < initial
    (initial0, once0), genie0 = _passes(0, m, which)
    print(f" 0 dB m = {m} {which}: initial {initial0:.4f}  one pass {once0:.4f}  genie {genie0:.3e}")


@pytest.mark.parametrize("m", (2, 4, 6, 8))
@pytest.mark.parametrize("R", (1, 2))
def test_the_decisions_are_the_diversity_links(R, m):
    """est = ideal at 30 dB: the symbol-error count is ``link_mrc_host``'s, the map decodes to the sent levels wherever that link
    counts no error, pilots read 255 and carry the frame's own pilot, and z is the channel plus noise over the decided symbol."""
    sim, tb, ideal, pilots, meta, keys, sigma = _frames(30, 8)
    cfg = LinkConfig(sim, m)
    rho, scale = branch_weights(meta[:, 0], 0.0, R)
    z, dec, errors = link_observe_host(cfg, keys, ideal, ideal, sigma, rho, pilots, R)
    counts, _, _, wrong, flags = link_mrc_host(cfg, keys, ideal, ideal, sigma, rho, scale, R, tau=1e-6)
    assert z.shape == ideal.shape and z.dtype == np.complex128 and dec.shape == (8 // R, *sim.ofdm) and dec.dtype == np.uint8
    assert errors.dtype == np.int64 and (errors == counts[:, 1]).all()
    mask = cfg.data_mask
    assert (dec[:, ~mask] == PILOT_DECISION).all()
    assert m == 8 or (dec[:, mask] != PILOT_DECISION).all()                      # at m = 8 the byte 255 is also the decision (15, 15)
    sc, sym = np.asarray(sim.pilot_scs), np.asarray(sim.pilot_symbols)
    assert (z[:, sc[:, None], sym[None, :]] == pilots).all()
    from adafortitran_amd.linksim import _sent
    gi, gq, x = _sent(cfg, keys[::R])
    right = (wrong == 0) & mask[None]
    assert ((dec & 15)[right] == gray_level(gi)[right]).all() and ((dec >> 4)[right] == gray_level(gq)[right]).all()
    # where the decision is right z - H is the noise over x: |z - H| |x| = |noise|
    from adafortitran_amd.linksim import _noise
    for r in range(R):
        noise = _noise(cfg, keys[r::R], sigma[r::R].astype(np.float64))
        assert np.allclose(((z[r::R] - ideal[r::R]) * x)[right], (noise * x.conj() / np.abs(x) ** 2 * x)[right], rtol=1e-9, atol=1e-12)
    # the flags are link_mrc_host's own
    assert (link_observe_host(cfg, keys, ideal, ideal, sigma, rho, pilots, R, tau=1e-6)[3] == flags).all()


def test_a_given_decision_map_round_trips_and_the_genie_is_the_sent_map():
    sim, tb, ideal, pilots, meta, keys, sigma = _frames(20, 8)
    cfg, rho = LinkConfig(sim, 4), np.ones(8, dtype=np.float32)
    est = lmmse_estimate_host(tb, pilots, meta).astype(np.complex64)
    z, dec, errors = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots)
    assert errors.sum() > 0
    z2, dec2, errors2 = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots, decisions=dec)
    assert (z2 == z).all() and (dec2 == dec).all() and (errors2 == errors).all()
    # the sent levels as a map: no symbol errors, and z is source="sent"'s
    from adafortitran_amd.linksim import _sent
    gi, gq, _ = _sent(cfg, keys)
    sent = np.where(cfg.data_mask[None], gray_level(gi) | (gray_level(gq) << 4), PILOT_DECISION).astype(np.uint8)
    z3, dec3, errors3 = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots, decisions=sent)
    zs, decs, errs = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots, source="sent")
    assert (errors3 == 0).all() and (dec3 == sent).all() and np.allclose(z3, zs, rtol=1e-12, atol=0)
    assert (decs == dec).all() and (errs == errors).all()                         # source="sent" keeps the decided map and count


def _loaders(sim, n=32, batch=16):
    packs = {snr: make_pack(sim, n, seed=20 + snr, snr_db=snr) for snr in (0, 20)}
    return packs, [(f"SNR_{snr}", ingest.ResidentLoader(p, sim.pilot, batch, device="cpu", shuffle=False)) for snr, p in packs.items()]


def test_the_refiner_and_the_sweeps_on_the_cpu_are_the_twins_applied_by_hand():
    sim = ChannelSimConfig()
    cfg, seed, m = LinkConfig(sim, 4), 5, 4
    packs, loaders = _loaders(sim)
    model = LmmseEstimator(sim)
    tb = LmmseTables(sim)
    plain, once, twice = (get_link_stats(model, loaders, cfg, seed=seed, refine=r) for r in (None, 1, 2))
    assert plain == get_link_stats(model, loaders, cfg, seed=seed) == get_link_stats(model, loaders, cfg, seed=seed, refine=0)
    nmse0, nmse1 = get_test_stats(model, loaders), get_refined_test_stats(model, loaders, cfg, refine=1, seed=seed)
    assert get_refined_test_stats(model, loaders, cfg, refine=0, seed=seed) == nmse0 and list(nmse1) == [0, 20]
    sc, sym = np.asarray(sim.pilot_scs), np.asarray(sim.pilot_symbols)
    from adafortitran_amd.linksim import link_errors_host
    for snr, pack in packs.items():
        n = len(pack["h_ideal"])
        keys, sigma, meta = frame_keys(seed, np.arange(n)), noise_sigma(pack["meta"][:, 1]), pack["meta"][:, 1:4]
        pilots = pack["h_ls_sparse"][:, sc[:, None], sym[None, :]]
        est = lmmse_estimate_host(tb, pilots, meta).astype(np.complex64)
        for want_ber, passes in ((once, 1), (twice, 2)):
            e = est
            for _ in range(passes):
                z, _, errors = link_observe_host(cfg, keys, pack["h_ideal"], e, sigma, np.ones(n, dtype=np.float32), pilots)
                e = lmmse_grid_host(tb, z, meta, noise_scale=data_noise_scale(m)).astype(np.complex64)
            counts = link_errors_host(cfg, keys, pack["h_ideal"], e, sigma)
            assert want_ber[snr] == counts[:, 0].sum() / (n * cfg.bits_per_frame)
            if passes == 1:
                mse = float((np.abs(e.astype(np.complex128) - pack["h_ideal"]) ** 2).mean())
                assert nmse1[snr] == pytest.approx(10 * np.log10(mse), abs=1e-4)
    print(f"BER plain {plain}  one pass {once}  two passes {twice};  NMSE dB plain {nmse0}  one pass {nmse1}")
    assert once[20] < plain[20] and nmse1[20] < nmse0[20]
    # the refiner by hand: iterations = 0 returns est ITSELF; a refiner handed to a sweep keeps counting; the error rate is the last pass's
    pilots_t, ideal_t, meta_t = next(iter(loaders[1][1]))
    est_t = model(pilots_t, meta_t)
    assert DataAidedRefiner(cfg, "cpu", seed, iterations=0).refine(est_t, pilots_t, ideal_t, meta_t) is est_t
    ref = DataAidedRefiner(cfg, "cpu", seed, iterations=1)
    assert ref.symbol_error_rate() == 0.0
    assert get_link_stats(model, loaders[1:], cfg, seed=seed, refine=ref) == {20: once[20]}
    n = len(packs[20]["h_ideal"])
    z, _, errors = link_observe_host(cfg, frame_keys(seed, np.arange(n)), packs[20]["h_ideal"],
                                     lmmse_estimate_host(tb, packs[20]["h_ls_sparse"][:, sc[:, None], sym[None, :]],
                                                         packs[20]["meta"][:, 1:4]).astype(np.complex64),
                                     noise_sigma(packs[20]["meta"][:, 1]), np.ones(n, dtype=np.float32),
                                     packs[20]["h_ls_sparse"][:, sc[:, None], sym[None, :]])
    assert ref.groups == n and ref.symbol_error_rate() == errors.sum() / (n * cfg.data_elements)
    genie = DataAidedRefiner(cfg, "cpu", seed, source="sent").refine(est_t, pilots_t, ideal_t, meta_t)
    assert _nmse(genie.numpy(), ideal_t.numpy()) < 0.01 * _nmse(est_t.numpy(), ideal_t.numpy())
    # the coded sweeps take the keyword too (one small loader each)
    ldpc = LdpcConfig(cfg, (3, 6))
    assert get_link_bler(model, loaders[1:], ldpc, seed=seed, refine=1)[20] <= get_link_bler(model, loaders[1:], ldpc, seed=seed)[20]
    assert get_link_rates(model, loaders[1:], cfg, seed=seed, refine=1)[20] > get_link_rates(model, loaders[1:], cfg, seed=seed)[20]


def test_two_branches_are_decided_together_and_refined_each():
    sim = ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3))
    cfg, seed, R = LinkConfig(sim, 4), 5, 2
    ideal, pilots, meta = simulate_frames_host(sim, seed, np.arange(8))
    tb = LmmseTables(sim)
    est = lmmse_estimate_host(tb, pilots, meta).astype(np.complex64)
    frames = (torch.from_numpy(est), torch.from_numpy(pilots.astype(np.complex64)), torch.from_numpy(ideal.astype(np.complex64)))
    got = DataAidedRefiner(cfg, "cpu", seed, branches=R).refine(*frames, frame_ids=np.arange(8), snr_db=meta[:, 0],
                                                               meta=(None, *(torch.from_numpy(meta[:, k].copy()) for k in range(3))))
    rho, _ = branch_weights(meta[:, 0], 0.0, R)
    z, dec, _ = link_observe_host(cfg, frame_keys(seed, np.arange(8)), frames[2].numpy(), est, noise_sigma(meta[:, 0]), rho,
                                  frames[1].numpy(), R)
    want = lmmse_grid_host(tb, z, meta, noise_scale=data_noise_scale(4)).astype(np.complex64)
    assert dec.shape[0] == 4 and (got.numpy() == want).all()


def test_with_branches_the_refiner_combines_with_the_accumulators_err_var():
    """The coded sweeps weight the branches by ``branch_weights(snr, err_var, R)``; a refiner built for them decides on the same sums."""
    sim = ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3))
    cfg, seed, R, err_var = LinkConfig(sim, 4), 5, 2, 0.05
    ideal, pilots, meta = simulate_frames_host(sim, seed, np.arange(8))
    tb = LmmseTables(sim)
    est = lmmse_estimate_host(tb, pilots, meta).astype(np.complex64)
    frames = (torch.from_numpy(est), torch.from_numpy(pilots.astype(np.complex64)), torch.from_numpy(ideal.astype(np.complex64)))
    metas = (torch.arange(8).float(), *(torch.from_numpy(meta[:, k].copy()) for k in range(3)))
    got = DataAidedRefiner(cfg, "cpu", seed, branches=R, err_var=err_var).refine(*frames, metas)
    rho, _ = branch_weights(meta[:, 0], err_var, R)
    assert (rho != branch_weights(meta[:, 0], 0.0, R)[0]).any()
    z, _, _ = link_observe_host(cfg, frame_keys(seed, np.arange(8)), frames[2].numpy(), est, noise_sigma(meta[:, 0]), rho, frames[1].numpy(), R)
    assert (got.numpy() == lmmse_grid_host(tb, z, meta, noise_scale=data_noise_scale(4)).astype(np.complex64)).all()
    assert as_refiner(1, cfg, "cpu", seed, R, err_var=err_var).err_var == err_var
    with pytest.raises(ValueError, match="err_var"):
        as_refiner(DataAidedRefiner(cfg, "cpu", seed, branches=R), cfg, "cpu", seed, R, err_var=err_var)
    with pytest.raises(ValueError, match="err_var"):
        DataAidedRefiner(cfg, "cpu", seed, err_var=-1.0)


def test_refusals():
    sim = ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3))
    cfg = LinkConfig(sim, 4)
    ideal, pilots, meta = simulate_frames_host(sim, 5, np.arange(4))
    keys, sigma, rho = frame_keys(5, np.arange(4)), noise_sigma(meta[:, 0]), np.ones(4, dtype=np.float32)
    with pytest.raises(ValueError, match='"decided"'):
        link_observe_host(cfg, keys, ideal, ideal, sigma, rho, pilots, source="soft")
    with pytest.raises(ValueError, match="pilots of shape"):
        link_observe_host(cfg, keys, ideal, ideal, sigma, rho, pilots[:, :4])
    with pytest.raises(ValueError, match="multiple of branches"):
        link_observe_host(cfg, keys, ideal, ideal, sigma, rho, pilots, branches=3)
    with pytest.raises(ValueError, match="decisions must be uint8"):
        link_observe_host(cfg, keys, ideal, ideal, sigma, rho, pilots, decisions=np.zeros((4, 30, 7), dtype=np.int64))
    with pytest.raises(ValueError, match="beyond the 4 levels"):
        link_observe_host(cfg, keys, ideal, ideal, sigma, rho, pilots, decisions=np.full((4, 30, 7), 7, dtype=np.uint8))
    with pytest.raises(ValueError, match="rho must hold"):
        link_observe_host(cfg, keys, ideal, ideal, sigma, rho[:3], pilots)
    with pytest.raises(ValueError, match="iterations"):
        DataAidedRefiner(cfg, "cpu", iterations=-1)
    with pytest.raises(ValueError, match="LinkConfig"):
        DataAidedRefiner(sim, "cpu")
    with pytest.raises(ValueError, match="at most 32"):
        DataAidedRefiner(LinkConfig(ChannelSimConfig(ofdm=(12, 33), pilot=(2, 2)), 2), "cpu")       # T = 33
    e = torch.from_numpy(ideal.astype(np.complex64))
    ref = DataAidedRefiner(cfg, "cpu", 5)
    with pytest.raises(ValueError, match="perfect channel knowledge"):
        ref.refine(None, torch.from_numpy(pilots.astype(np.complex64)), e, frame_ids=np.arange(4), snr_db=20.0)
    with pytest.raises(ValueError, match="pilots must be complex64"):
        ref.refine(e, torch.from_numpy(pilots), e, frame_ids=np.arange(4), snr_db=20.0)
    with pytest.raises(ValueError, match="delay_spread_ns"):
        ref.refine(e, torch.from_numpy(pilots.astype(np.complex64)), e, frame_ids=np.arange(4), snr_db=20.0)
    # the sweeps: what works is named
    model = LmmseEstimator(sim)
    for kw in (dict(streams=2, branches=2), dict(tx_diversity="time"), dict(precoding_subband=5)):
        with pytest.raises(ValueError, match="single-stream link.*branches"):
            get_link_stats(model, [], cfg, refine=1, **kw)
        with pytest.raises(ValueError, match="single-stream link"):
            get_link_rates(model, [], cfg, refine=1, **kw)
    for bad in (-1, 1.5, True, "1"):
        with pytest.raises(ValueError, match="iteration count"):
            get_link_stats(model, [], cfg, refine=bad)
    with pytest.raises(ValueError, match="another link, seed"):
        get_link_stats(model, [], cfg, seed=1, refine=DataAidedRefiner(cfg, "cpu", seed=2))
    with pytest.raises(ValueError, match="refine = None"):
        get_refined_test_stats(model, [], cfg, refine=None)
    assert as_refiner(None, cfg, "cpu") is None
    _, loaders = _loaders(ChannelSimConfig(), 16)
    with pytest.raises(ValueError, match="perfect channel knowledge"):
        get_link_stats(None, loaders[:1], LinkConfig(ChannelSimConfig(), 4), refine=1)


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    assert "aft_link_observe_f32" in _abi.SIGNATURES and "aft_link_observe_f32" in _abi.EXPORTED_SYMBOLS
    restype, argtypes = _abi.SIGNATURES["aft_link_observe_f32"]
    assert len(argtypes) == 14 and _abi.AFT_ABI_VERSION == 10
    assert (_abi.AFT_LINK_OBSERVE_DECIDED, _abi.AFT_LINK_OBSERVE_SENT) == (0, 1)
