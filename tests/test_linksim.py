"""``adafortitran_amd.linksim`` on the CPU: the definition of the link-level error count (constellation, Gray map, the two exact
extremes, pilot positions excluded, the Rayleigh closed form, the order perfect < LMMSE < LS), the share of flagged decisions on the
inputs tests/test_linksim_gpu.py compares the kernel on, ``LinkAccumulator`` / ``get_link_stats`` on the host and over two gloo ranks,
the ``aft_link`` mirror against the header.

``link_inputs`` builds those inputs once per grid; the GPU file imports it, so both files speak about the same arrays."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from adafortitran_amd import _abi, ingest
from adafortitran_amd.chansim import (ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, make_pack,
                                      simulate_frames_host)
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, STREAM_DATA_BITS, STREAM_DATA_NOISE_ANGLE, STREAM_DATA_NOISE_RADIUS,
                                      LinkAccumulator, LinkConfig, constellation, frame_keys_torch, gray_level, link_errors_host,
                                      noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator, LmmseTables, lmmse_estimate_host

SEED = 3
TAU_CAP, SHARE_CAP = 1e-5, 1e-3          # the issue's: tau at most 1e-5, at most 1e-3 of the (element, axis) pairs flagged there

# grid, pilots, frames: the smallest shapes at which the kernel can go wrong (tests/test_linksim_gpu.py says what each exercises)
GRIDS = {
    "default_120x14": (ChannelSimConfig(), 3),
    "odd_30x7": (ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3)), 5),
    "pilot_bounds_128x40": (ChannelSimConfig(ofdm=(128, 40), pilot=(64, 16)), 2),
    "one_data_element_2x1": (ChannelSimConfig(ofdm=(2, 1), pilot=(1, 1)), 1),
    "no_data_element_1x1": (ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), 1),
    "odd_last_alone_3x5": (ChannelSimConfig(ofdm=(3, 5), pilot=(1, 1)), 2),     # pilot at (1, 2); element 14 is data, alone in its pair
}
_inputs = {}


def link_inputs(name):
    """(sim, keys uint64 [n], sigma float32 [n], ideal complex64 [n,S,T], {"lmmse": .., "ideal": ..} estimates complex64), made once per
    grid and read-only: frames [0, n) of seed 3 from the float64 simulator, each at the SNR it was drawn with."""
    if name not in _inputs:
        sim, n = GRIDS[name]
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(n))
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        est = {"lmmse": lmmse_estimate_host(sim, pilots, meta).astype(np.complex64), "ideal": ideal}
        keys, sigma = frame_keys(SEED, np.arange(n)), noise_sigma(meta[:, 0])
        for a in (ideal, est["lmmse"], keys, sigma):
            a.setflags(write=False)
        _inputs[name] = (sim, keys, sigma, ideal, est)
    return _inputs[name]


def flagged_share(cfg, flags):
    pairs = 2 * cfg.data_elements * len(flags)
    return float(flags.sum()) / pairs if pairs else 0.0


def test_streams_continue_the_simulators_and_the_config_validates():
    from adafortitran_amd import chansim
    assert (STREAM_DATA_BITS, STREAM_DATA_NOISE_RADIUS, STREAM_DATA_NOISE_ANGLE) == (5, 6, 7)
    assert max(chansim.STREAM_CONDITION, chansim.STREAM_ANGLE, chansim.STREAM_PHASE, chansim.STREAM_NOISE_RADIUS,
               chansim.STREAM_NOISE_ANGLE) == 4
    cfg = LinkConfig()
    assert cfg.bits_per_symbol == 4 and cfg.levels == 4 and cfg.sim.ofdm == (120, 14)
    assert cfg.data_elements == 1680 - 24 and cfg.bits_per_frame == 4 * 1656 and cfg.data_mask.sum() == 1656
    for bad in (0, 1, 3, 10, -2, 4.0, "4", True):
        with pytest.raises(ValueError, match="bits_per_symbol"):
            LinkConfig(ChannelSimConfig(), bad)
    with pytest.raises(ValueError, match="ChannelSimConfig"):
        LinkConfig((120, 14), 4)
    with pytest.raises(ValueError, match="2\\^31"):
        LinkConfig(ChannelSimConfig(ofdm=(1 << 16, (1 << 15) + 1)), 2)
    assert noise_sigma(10.0).dtype == np.float32
    assert noise_sigma(ChannelSimConfig().snr_db).tobytes() == ChannelSimConfig().tables()["noise_sigma"].tobytes()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_constellation_has_unit_mean_energy_and_a_gray_map(m):
    pts = constellation(m)
    L = 1 << (m // 2)
    assert len(pts) == 1 << m and len(set(np.round(pts, 12))) == 1 << m
    assert abs(float((np.abs(pts) ** 2).mean()) - 1.0) <= 1e-12
    d = LinkConfig(bits_per_symbol=m).d
    assert sorted(set(np.round(pts.real / d).astype(int))) == list(range(-(L - 1), L, 2))
    # the Gray code of level k is k ^ (k >> 1), gray_level is its inverse, and neighbouring levels differ in exactly one bit
    k = np.arange(L)
    g = k ^ (k >> 1)
    assert gray_level(g).tolist() == k.tolist() and sorted(g.tolist()) == k.tolist()
    assert all(bin(int(a ^ b)).count("1") == 1 for a, b in zip(g, g[1:]))
    # ... so the nearest neighbours of a symbol differ from it in one bit of its word
    for w in range(1 << m):
        near = [v for v in range(1 << m) if v != w and abs(abs(pts[v] - pts[w]) - 2 * d) <= 1e-12]
        assert 2 <= len(near) <= 4 and all(bin(v ^ w).count("1") == 1 for v in near)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_two_exact_extremes(m):
    for name in ("default_120x14", "odd_30x7", "one_data_element_2x1", "no_data_element_1x1", "odd_last_alone_3x5"):
        sim, keys, sigma, ideal, _ = link_inputs(name)
        cfg = LinkConfig(sim, m)
        zero = np.zeros_like(sigma)
        if name == "odd_last_alone_3x5":           # the MSB of each axis flips at every m; a dropped last element would read (26, 13)
            assert cfg.data_elements == 14 and cfg.data_mask[2, 4] and not cfg.data_mask[1, 2] and np.abs(ideal).min() > 0.5
            assert link_errors_host(cfg, keys, ideal, -ideal, zero).tolist() == [[28, 14]] * 2
        counts, wrong, flags = link_errors_host(cfg, keys, ideal, ideal, zero, tau=TAU_CAP)
        assert counts.dtype == np.int64 and counts.shape == (len(keys), 2)
        assert not counts.any() and not wrong.any() and not flags.any()          # the estimate is the channel and there is no noise
        if m == 2:                                                               # the estimate points the other way: every bit flips
            counts, wrong, flags = link_errors_host(cfg, keys, ideal, -ideal, zero, tau=TAU_CAP)
            assert (counts[:, 0] == 2 * cfg.data_elements).all() and (counts[:, 1] == cfg.data_elements).all()
            assert not flags.any()
    with pytest.raises(ValueError, match="shape"):
        link_errors_host(cfg, keys, ideal[:, :0], ideal, zero)
    with pytest.raises(ValueError, match="one value per frame"):
        link_errors_host(cfg, keys, ideal, ideal, np.zeros(3))
    with pytest.raises(ValueError, match="64-bit"):
        link_errors_host(cfg, keys.astype(np.float64), ideal, ideal, zero)


def test_pilot_positions_are_excluded():
    """Irregular pilot rows and columns, every data bit wrong: the error map is 2 off the pilots' cross product and 0 on it."""
    sim = ChannelSimConfig(pilot=(4, 3), pilot_scs=(0, 7, 118, 119), pilot_symbols=(0, 1, 13))
    cfg = LinkConfig(sim, 2)
    ideal = simulate_frames_host(sim, SEED, np.arange(2))[0].astype(np.complex64)
    counts, wrong, _ = link_errors_host(cfg, frame_keys(SEED, np.arange(2)), ideal, -ideal, np.zeros(2, np.float32), tau=TAU_CAP)
    want = np.full((120, 14), 2)
    for s in (0, 7, 118, 119):
        for t in (0, 1, 13):
            want[s, t] = 0
    assert (wrong == want[None]).all() and (want == 0).sum() == 12
    assert counts.tolist() == [[2 * (1680 - 12), 1680 - 12]] * 2
    assert (cfg.data_mask == (want == 2)).all()


_frames600 = {}


def _pinned_snr_frames(snr_db, n=600):
    if snr_db not in _frames600:
        sim = ChannelSimConfig(snr_db=(float(snr_db),))
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(n))
        _frames600[snr_db] = (sim, ideal.astype(np.complex64), pilots.astype(np.complex64), meta, frame_keys(SEED, np.arange(n)),
                              noise_sigma(meta[:, 0]))
    return _frames600[snr_db]


@pytest.mark.parametrize("snr_db", (0, 10))
def test_qpsk_with_perfect_csi_follows_the_rayleigh_closed_form(snr_db):
    """BER = (1 - sqrt(g / (1 + g))) / 2 with g = 1 / (2 sigma^2) per bit; the sum-of-sinusoids channel is only approximately
    Gaussian, 600 frames, 10 % relative.  (Not at 20 dB: the sample is too small there.)"""
    sim, ideal, _, _, keys, sigma = _pinned_snr_frames(snr_db)
    cfg = LinkConfig(sim, 2)
    counts = link_errors_host(cfg, keys, ideal, ideal, sigma)
    ber = counts[:, 0].sum() / (len(keys) * cfg.bits_per_frame)
    g = 1.0 / (2.0 * float(sigma[0]) ** 2)
    want = 0.5 * (1.0 - np.sqrt(g / (1.0 + g)))
    print(f"{snr_db} dB: BER {ber:.4f}  closed form {want:.4f}")
    assert abs(ber - want) <= 0.10 * want


def test_perfect_csi_beats_lmmse_beats_ls_interpolation_at_10_db():
    sim, ideal, pilots, meta, keys, sigma = _pinned_snr_frames(10)
    cfg = LinkConfig(sim, 2)
    ests = (ideal, lmmse_estimate_host(sim, pilots, meta).astype(np.complex64), ls_interpolate(sim, pilots))
    ber = [link_errors_host(cfg, keys, ideal, e, sigma)[:, 0].sum() / (len(keys) * cfg.bits_per_frame) for e in ests]
    print("BER perfect / LMMSE / LS:", [round(float(v), 4) for v in ber])
    assert ber[0] < ber[1] < ber[2]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_few_decisions_are_flagged_on_the_inputs_the_gpu_tests_use(m):
    """The comparison rule of tests/test_linksim_gpu.py lets a flagged decision go either way, so it says something only while few
    are flagged: at most 1e-3 of the (element, axis) pairs at tau = 1e-5, for every input set used there."""
    worst = 0.0
    for name in GRIDS:
        sim, keys, sigma, ideal, est = link_inputs(name)
        cfg = LinkConfig(sim, m)
        for which, e in est.items():
            share = flagged_share(cfg, link_errors_host(cfg, keys, ideal, e, sigma, tau=TAU_CAP)[2])
            worst = max(worst, share)
            assert share <= SHARE_CAP, (name, which, share)
    # the accumulator's sweep there: five batches of 16 from SynthLoader, seed 2 (the host twin of the device's frames)
    sim = ChannelSimConfig()
    cfg, tb = LinkConfig(sim, m), LmmseTables(sim)
    for pil, ideal, meta in SynthLoader(sim, 16, 80, device="cpu", seed=2):
        g = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
        cond = np.concatenate([t.numpy() for t in meta[1:4]], axis=1)
        lm = lmmse_estimate_host(tb, pil.numpy(), cond).astype(np.complex64)
        for e in (lm, ideal.numpy()):
            share = flagged_share(cfg, link_errors_host(cfg, frame_keys(2, g), ideal.numpy(), e, noise_sigma(cond[:, 0]), tau=TAU_CAP)[2])
            worst = max(worst, share)
            assert share <= SHARE_CAP
    print(f"m = {m}: largest flagged share at tau = {TAU_CAP:g}: {worst:.2e}")


def test_frame_keys_with_torch_ops_are_the_simulators():
    g = np.array([0, 1, 2, 77, (1 << 24) - 1, (1 << 40) + 5], dtype=np.int64)
    for seed in (0, 3, -1, (1 << 63) + 11):
        got = frame_keys_torch(seed, torch.from_numpy(g)).numpy().view(np.uint64)
        assert (got == frame_keys(seed, g)).all()
    as_float = frame_keys_torch(3, torch.from_numpy(g[:5]).to(torch.float32).reshape(-1, 1)).numpy().view(np.uint64)
    assert (as_float == frame_keys(3, g[:5])).all()                       # file_no as the loaders carry it: exact below 2^24


def _loaders(sim):
    packs = {snr: make_pack(sim, 48, seed=20 + snr, snr_db=snr) for snr in (0, 20)}
    return packs, [(f"SNR_{snr}", ingest.ResidentLoader(p, sim.pilot, 16, device="cpu", shuffle=False)) for snr, p in packs.items()]


def test_accumulator_and_sweep_on_the_cpu_over_two_loaders():
    from adafortitran_amd.evaluation import get_link_stats
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    packs, loaders = _loaders(sim)
    model = LmmseEstimator(sim)
    perfect, lmmse = get_link_stats(None, loaders, cfg, seed=5), get_link_stats(model, loaders, cfg, seed=5)
    assert list(perfect) == list(lmmse) == [0, 20]
    sc, sym = np.asarray(sim.pilot_scs), np.asarray(sim.pilot_symbols)
    for snr, pack in packs.items():
        keys, sigma = frame_keys(5, np.arange(48)), noise_sigma(pack["meta"][:, 1])
        est = lmmse_estimate_host(sim, pack["h_ls_sparse"][:, sc[:, None], sym[None, :]], pack["meta"][:, 1:4]).astype(np.complex64)
        for got, e in ((perfect[snr], pack["h_ideal"]), (lmmse[snr], est)):
            counts = link_errors_host(cfg, keys, pack["h_ideal"], e, sigma)
            assert got == counts[:, 0].sum() / (48 * cfg.bits_per_frame)
        assert perfect[snr] < lmmse[snr]
    assert perfect[20] < perfect[0] and lmmse[20] < lmmse[0]
    # the accumulator by hand: explicit frame numbers and one SNR for the batch, symbol errors, an empty sweep
    acc = LinkAccumulator(cfg, "cpu", seed=5)
    ideal = torch.from_numpy(packs[0]["h_ideal"])
    acc.update(None, ideal[:10], frame_ids=np.arange(10), snr_db=0.0)
    acc.update(ideal[10:], ideal[10:], frame_ids=torch.arange(10, 48), snr_db=torch.zeros(38))
    assert acc.frames == 48 and acc.result() == perfect[0]
    counts = link_errors_host(cfg, frame_keys(5, np.arange(48)), packs[0]["h_ideal"], packs[0]["h_ideal"], noise_sigma(np.zeros(48)))
    assert acc.result_ser() == counts[:, 1].sum() / (48 * cfg.data_elements)
    assert acc.local_pair().tolist() == [float(counts[:, 0].sum()), 48.0 * cfg.bits_per_frame]
    assert LinkAccumulator(cfg, "cpu").result() == 0.0
    with pytest.raises(ValueError, match="frame numbers"):
        acc.update(None, ideal[:2])
    with pytest.raises(ValueError, match="SNR"):
        acc.update(None, ideal[:2], frame_ids=[0, 1])
    with pytest.raises(ValueError, match="complex64"):
        acc.update(None, ideal[:2].to(torch.complex128), frame_ids=[0, 1], snr_db=0)
    with pytest.raises(ValueError, match="one frame number per frame"):
        acc.update(None, ideal[:2], frame_ids=[0, 1, 2], snr_db=0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    sim = ChannelSimConfig(snr_db=(10.0,))
    acc = LinkAccumulator(LinkConfig(sim, 4), "cpu", seed=SEED)
    for _, ideal, meta in SynthLoader(sim, 8, 40, device="cpu", seed=SEED, rank=rank, world_size=world, fresh_each_epoch=False):
        acc.update(None, ideal, meta)
    ret[rank] = (acc.result(), acc.result_ser(), acc.frames)
    dist.destroy_process_group()


def test_two_gloo_ranks_report_the_same_rates_bit_for_bit():
    world = 2
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
        results = dict(ret)
    assert results[0][:2] == results[1][:2] and results[0][2] + results[1][2] == 40
    sim = ChannelSimConfig(snr_db=(10.0,))
    cfg = LinkConfig(sim, 4)
    ideal = simulate_frames_host(sim, SEED, np.arange(40))[0].astype(np.complex64)
    counts = link_errors_host(cfg, frame_keys(SEED, np.arange(40)), ideal, ideal, noise_sigma(np.full(40, 10.0)))
    assert results[0][0] == counts[:, 0].sum() / (40 * cfg.bits_per_frame)
    assert results[0][1] == counts[:, 1].sum() / (40 * cfg.data_elements)


def test_struct_mirror_matches_the_header_and_the_abi_version_stays():
    """``aft_link``'s size and what ``to_struct`` puts into it; tests/test_abi.py checks the mirror against the header field by field."""
    assert ctypes.sizeof(_abi.AftLink) == 4 * (6 + 64 + 16)
    assert _abi.AFT_ABI_VERSION == 10 and "aft_link_errors_f32" in _abi.SIGNATURES
    p = LinkConfig(ChannelSimConfig(pilot=(4, 3), pilot_scs=(0, 7, 118, 119), pilot_symbols=(0, 1, 13)), 6).to_struct()
    assert (p.num_scs, p.num_symbols, p.pilot_scs, p.pilot_symbols, p.bits_per_symbol, p.reserved) == (120, 14, 4, 3, 6, 0)
    assert list(p.pilot_sc_index)[:5] == [0, 7, 118, 119, 0] and list(p.pilot_symbol_index)[:4] == [0, 1, 13, 0]
