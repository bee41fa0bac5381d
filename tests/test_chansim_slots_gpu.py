"""``aft_channel_sim_seq_f32`` (slot sequences: chansim.py, "time continuity") on the HIP device: the sequence kernel against the float64
definition within a bound DERIVED from the configuration, meta bit for bit, no unwritten output; ``slots=1`` against the grouped and
the ungrouped entry points bit for bit, slot 0 of a sequence against the group of the same number bit for bit, batch / position /
shard independence bit for bit, the checked build, the entry point's refusals, and the loader against its CPU twin without a
synchronisation.

The bound restates ``derived_bounds`` of tests/test_chansim_gpu.py (its docstring has the derivation and the symbols u, A, M, P) with the
one term the slot adds, and ``derived_bounds_grouped`` of tests/test_chansim_groups_gpu.py on top of it.  The slot's start phase is
phi_k = frac(fma(rate, float(k L), phi)): k L is exact, the product carries the rate's error k L d_rate, the fused multiply-add rounds a
value of at most A k L + 1 once, and x - floor(x) is exact for x >= 1 and rounds a value below 1 by at most u / 2 otherwise, which the
same term covers (|x| < 1 there):

    |d phi_k| <= k L d_rate + u (A k L + 1),        k <= K - 1

added into d_theta, the error of the phase in turns; everything downstream is unchanged.  Observed maxima are printed."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, simulate_frames_host
from adafortitran_amd.hip_ops import ChannelSimPlan, pack_mix
from test_chansim_gpu import DEV, U, _bits, _no_sync, _poison, _same_bits, _shapes

pytestmark = pytest.mark.gpu
FAR = 1 << 40
FULL3 = np.array([[1.0, 0.5 + 0.3j, 0.1 - 0.2j], [0.5 - 0.3j, 1.0, 0.4 + 0.1j], [0.1 + 0.2j, 0.4 - 0.1j, 1.0]])


def derived_bounds_seq(cfg: ChannelSimConfig):
    """(bound on |ideal - definition|, bound on |pilots - definition|) of a sequence configuration; module docstring."""
    t = cfg.tables()
    S, T = cfg.ofdm
    M, P = cfg.rays, len(t["tap_delay"])
    A = float(t["doppler_turns"].max())
    X = (S - 1) * float(t["delay_turns"].max()) * float(t["tap_delay"].max())
    gamma = M * float(t["tap_amp"].astype(np.float64).sum())
    r2 = np.sqrt(2.0)
    first = (cfg.slots - 1) * cfg.slot_symbols                  # the largest k L

    def channel(t_max):
        d_rate = A * ((2 * np.pi + 4) * U + U)
        d_theta = t_max * d_rate + U * (A * t_max + 1)
        d_theta += first * d_rate + U * (A * first + 1)         # the slot's start phase
        e_ray = 2 * np.pi * d_theta + 4 * r2 * U
        e_del = 4 * np.pi * U * X + 4 * r2 * U
        return gamma * (e_ray + r2 * M * U + e_del + 2 * r2 * P * U)

    r = float(t["noise_sigma"].max()) * np.sqrt(24 * np.log(2.0))
    noise_own = r * (4 * U + 4 * r2 * U)
    # the grouped extension (the sequence kernel mixes even one source: L = (1)): Lambda, n = G sources
    lam = float(np.abs(t["mix"].astype(np.complex128)).sum(axis=1).max())
    mixing = 2 * r2 * cfg.group * U * lam * gamma
    return (lam * channel(T - 1) + mixing,
            lam * channel(max(cfg.pilot_symbols)) + mixing + noise_own + r2 * U * (lam * gamma + r))


CONFIGS = {
    "default_120x14_K3": ChannelSimConfig(slots=3),
    "odd_30x7_K2_2x2": ChannelSimConfig(ofdm=(30, 7), pilot=(3, 1), slots=2, antennas=(2, 2), rx_correlation=0.7,
                                        tx_correlation=0.6 * np.exp(0.9j)),
    "long_72x80_K2": ChannelSimConfig(ofdm=(72, 80), pilot=(6, 4), slots=2),
    "gap_30x7_K3_L12": ChannelSimConfig(ofdm=(30, 7), pilot=(3, 1), slots=3, slot_symbols=12, antennas=(3, 1), rx_correlation=FULL3),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_sequence_kernel_against_the_float64_definition(name):
    cfg = CONFIGS[name]
    KG = cfg.sequence()
    plan = ChannelSimPlan(cfg, DEV)
    b_ideal, b_pilots = derived_bounds_seq(cfg)
    worst = [0.0, 0.0]
    for seed, base, seqs in ((1, 0, 1), (2, (1 << 33) + 3, 5)):
        batch = seqs * KG
        _poison(_shapes(cfg, batch))
        ideal, pilots, meta = plan(seed, base, 0, 1, FAR, batch)
        frames = base * KG + np.arange(batch)
        want_i, want_p, want_m = simulate_frames_host(cfg, seed, frames)
        assert ideal.shape == want_i.shape and pilots.shape == want_p.shape and ideal.dtype == pilots.dtype == torch.complex64
        assert torch.equal(_bits(meta), _bits(torch.from_numpy(want_m)))
        got_i, got_p = ideal.cpu().numpy().astype(np.complex128), pilots.cpu().numpy().astype(np.complex128)
        assert np.isfinite(got_i).all() and np.isfinite(got_p).all()             # nothing left unwritten
        worst = [max(worst[0], float(np.abs(got_i - want_i).max())), max(worst[1], float(np.abs(got_p - want_p).max()))]
    print(f"{name}: max|ideal - def| {worst[0]:.3e} (derived bound {b_ideal:.3e})   max|pilots - def| {worst[1]:.3e} (derived bound "
          f"{b_pilots:.3e})")
    assert worst[0] <= b_ideal and worst[1] <= b_pilots


def _seq_entry(lib, cfg, slots, slot_symbols, seed, base, start, stride, modulo, batch):
    """The sequence entry point itself, with any slots (the plan only takes it with slots > 1)."""
    outs = [torch.empty(s, dtype=dt, device=DEV) for s, dt in _shapes(cfg, batch)]
    for t in outs:
        (torch.view_as_real(t) if t.is_complex() else t).fill_(float("nan"))
    mix = pack_mix(cfg.mix())
    _lib.check(lib.aft_channel_sim_seq_f32(cfg.to_struct(), *cfg.antennas, mix.ctypes.data, slots, slot_symbols, seed, base, start, stride,
                                           modulo, batch, *(t.data_ptr() for t in outs), _lib.current_stream_ptr(outs[0].device)), lib)
    return outs


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_slot_is_the_grouped_kernel_and_slot_0_its_group_bit_for_bit(name):
    cfg = CONFIGS[name]
    one = dataclasses.replace(cfg, slots=1, slot_symbols=None)
    G, K, L, lib = cfg.group, cfg.slots, cfg.slot_symbols, _lib.load()
    # K = 1 through the sequence entry point: the grouped entry point's bits, and the ungrouped one's at G = 1
    got = _seq_entry(lib, one, 1, L, 5, 7, 1, 2, 50, 6 * G)
    _same_bits(got, _grouped_entry(lib, one, 5, 7, 1, 2, 50, 6 * G))
    _same_bits(got, ChannelSimPlan(one, DEV)(5, 7, 1, 2, 50, 6 * G))             # the plan's launch: grouped, or ungrouped at G = 1
    # slot 0 of sequence q is group q K of the one-slot configuration; a later slot is not the next group
    seqs = 4
    _poison(_shapes(cfg, seqs * K * G))
    whole = ChannelSimPlan(cfg, DEV)(5, 9, 0, 1, FAR, seqs * K * G)
    groups = ChannelSimPlan(one, DEV)(5, 9 * K, 0, 1, FAR, seqs * K * G)         # groups 9 K .. 9 K + seqs K - 1 (frames when G = 1)
    by_seq = [w.view(seqs, K, G, *w.shape[1:]) for w in whole]
    by_group = [w.view(seqs, K, G, *w.shape[1:]) for w in groups]
    _same_bits([w[:, 0].contiguous() for w in by_seq[:2]], [w[:, 0].contiguous() for w in by_group[:2]])
    assert not torch.equal(by_seq[0][:, 1], by_group[0][:, 1])
    m = by_seq[2]
    assert torch.equal(m, m[:, :1, :1].expand_as(m))                             # one set of conditions per sequence


def _grouped_entry(lib, cfg, seed, base, start, stride, modulo, batch):
    outs = [torch.empty(s, dtype=dt, device=DEV) for s, dt in _shapes(cfg, batch)]
    mix = pack_mix(cfg.mix())
    _lib.check(lib.aft_channel_sim_group_f32(cfg.to_struct(), *cfg.antennas, mix.ctypes.data, seed, base, start, stride, modulo, batch,
                                             *(t.data_ptr() for t in outs), _lib.current_stream_ptr(outs[0].device)), lib)
    return outs


@pytest.mark.parametrize("name", ["default_120x14_K3", "odd_30x7_K2_2x2", "long_72x80_K2"])
def test_a_sequence_does_not_depend_on_its_batch_its_position_or_its_rank(name):
    cfg = CONFIGS[name]
    KG, seqs = cfg.sequence(), 12
    plan = ChannelSimPlan(cfg, DEV)
    _poison(_shapes(cfg, KG * seqs))
    whole = plan(5, 0, 0, 1, FAR, KG * seqs)
    by_seq = [w.view(seqs, KG, *w.shape[1:]) for w in whole]
    for rank in range(3):                                                        # three shards of an epoch of 12 sequences
        share = plan(5, 0, rank, 3, 12, KG * 4)
        _same_bits(share, [w[rank::3].reshape(KG * 4, *w.shape[2:]) for w in by_seq])
    parts = [plan(5, 0, lo, 1, FAR, KG * 2) for lo in range(0, seqs, 2)]         # batches of 2 sequences
    _same_bits([torch.cat([p[k] for p in parts]) for k in range(3)], whole)
    _same_bits(plan(5, 9, 0, 1, FAR, KG * 3), [w[KG * 9:] for w in whole])       # base counts sequences
    wrapped = plan(5, 0, 10, 3, 12, KG * 3)                                      # sequence positions 10, 13, 16 -> 10, 1, 4
    _same_bits(wrapped, [w[[10, 1, 4]].reshape(KG * 3, *w.shape[2:]) for w in by_seq])
    _same_bits(plan(5, 0, 0, 1, FAR, KG * seqs), whole)                          # a second run


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_channel_sim_seq_f32"):    # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_channel_sim_seq_f32")
    for name, cfg in CONFIGS.items():
        plan = ChannelSimPlan(cfg, DEV)
        batch = 3 * cfg.sequence()
        _same_bits(plan(9, 3, 1, 2, 77, batch, lib=lib), plan(9, 3, 1, 2, 77, batch))
        one = dataclasses.replace(cfg, slots=1, slot_symbols=None)
        _same_bits(_seq_entry(lib, one, 1, cfg.slot_symbols, 9, 3, 1, 2, 77, 3 * cfg.group),
                   _seq_entry(_lib.load(), one, 1, cfg.slot_symbols, 9, 3, 1, 2, 77, 3 * cfg.group))


def test_every_refusal_of_the_entry_point_launches_nothing():
    lib, cfg = _lib.load(), CONFIGS["odd_30x7_K2_2x2"]
    KG = cfg.sequence()
    b = 2 * KG
    outs = [torch.empty(s, dtype=dt, device=DEV) for s, dt in _shapes(cfg, b)]
    for t in outs:
        (torch.view_as_real(t) if t.is_complex() else t).fill_(float("nan"))
    ptr = [t.data_ptr() for t in outs]
    mix = pack_mix(cfg.mix())

    def refused(code, word, sim=None, rx=2, tx=2, mixp=mix.ctypes.data, slots=2, slot_symbols=7, seed=1, base=0, start=0, stride=1,
                modulo=10, batch=b, ideal=ptr[0], pilots=ptr[1], meta=ptr[2]):
        rc = lib.aft_channel_sim_seq_f32(sim if sim is not None else cfg.to_struct(), rx, tx, mixp, slots, slot_symbols, seed, base, start,
                                         stride, modulo, batch, ideal, pilots, meta, None)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    rc = lib.aft_channel_sim_seq_f32(None, 2, 2, mix.ctypes.data, 2, 7, 1, 0, 0, 1, 10, b, *ptr, None)
    assert rc == E and "NULL" in lib.aft_last_error().decode()
    for k in ("ideal", "pilots", "meta", "mixp"):
        refused(E, "NULL", **{k: None})
    refused(E, "8-byte", ideal=ptr[0] + 4)
    refused(E, "4-byte", meta=ptr[2] + 2)
    refused(E, "4-byte", mixp=mix.ctypes.data + 2)
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for batch in (KG - 4, KG + 4, 4):                                            # whole groups, not whole sequences
        refused(E, f"batch = {batch} is not a multiple of slots * rx * tx = 2 * 2 * 2", batch=batch)
    for kw in (dict(base=-1), dict(start=-1), dict(stride=0), dict(modulo=0), dict(base=(1 << 62) // KG),
               dict(start=1 << 58, stride=1 << 58)):
        refused(E, "bad frame numbers", **kw)
    for kw, word in ((dict(slots=0), "slots = 0"), (dict(slots=-1), "slots = -1"), (dict(slots=4097), "slots = 4097"),
                     (dict(slot_symbols=6), "slot_symbols = 6"), (dict(slot_symbols=4097), "slot_symbols = 4097"),
                     (dict(slots=8, slot_symbols=513, batch=8 * 4), "slots * slot_symbols = 4104"),
                     (dict(rx=0), "rx = 0"), (dict(rx=5, tx=4), "rx * tx = 20")):
        refused(SH, word, **kw)
    sim = cfg.to_struct()
    sim.taps = 33
    refused(SH, "taps = 33", sim=sim)
    bad = mix.copy()
    bad[3] = np.inf
    refused(E, "mix[3]", mixp=bad.ctypes.data)
    torch.cuda.synchronize()
    assert all(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all() for t in outs)      # nothing was launched
    assert lib.aft_channel_sim_seq_f32(cfg.to_struct(), 2, 2, mix.ctypes.data, 2, 7, 1, 0, 0, 1, 10, b, *ptr, None) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert all(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all() for t in outs)   # ... and the good call writes it all
    _same_bits(outs, ChannelSimPlan(cfg, DEV)(1, 0, 0, 1, 10, b))


@pytest.mark.parametrize("world,fresh,drop_last", [(1, True, False), (2, False, True)])
def test_loader_on_the_device_matches_its_cpu_twin_without_a_synchronisation(world, fresh, drop_last):
    cfg = CONFIGS["odd_30x7_K2_2x2"]
    KG = cfg.sequence()
    b_ideal, b_pilots = derived_bounds_seq(cfg)
    t = cfg.tables()
    lam = float(np.abs(t["mix"].astype(np.complex128)).sum(axis=1).max())
    gamma = cfg.rays * float(t["tap_amp"].astype(np.float64).sum())
    r = float(t["noise_sigma"].max()) * np.sqrt(24 * np.log(2.0))
    kw = dict(batch_size=2 * KG, frames_per_epoch=7 * KG, seed=4, rank=world - 1, world_size=world, drop_last=drop_last, fresh_each_epoch=fresh)
    dev, host = SynthLoader(cfg, device=DEV, **kw), SynthLoader(cfg, device="cpu", **kw)
    assert len(dev) == len(host) and type(dev._plan) is ChannelSimPlan and dev._plan.slots == 2
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                                                         # the mode is honoured
        epochs = [list(dev) for _ in range(2)]
    for got in epochs:
        want = list(host)
        assert len(got) == len(want) == len(dev) and len(got) > 0
        for (pd, idv, md), (ph, ih, mh) in zip(got, want):
            assert pd.is_cuda and idv.is_cuda and pd.shape == ph.shape and idv.shape == ih.shape and idv.shape[0] % KG == 0
            assert all(torch.equal(x, y) for x, y in zip(md[:5], mh[:5])) and md[5] == mh[5]
            # the twin's batch is the definition ROUNDED to complex64
            assert float((idv.cpu() - ih).abs().max()) <= b_ideal + np.sqrt(2.0) * U * lam * gamma
            assert float((pd.cpu() - ph).abs().max()) <= b_pilots + np.sqrt(2.0) * U * (lam * gamma + r)
