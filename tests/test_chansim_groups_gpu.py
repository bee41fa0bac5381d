"""``aft_channel_sim_group_f32`` (antenna correlation: chansim.py, "Kronecker frame groups") on the HIP device: the grouped kernel
against the float64 definition within a bound DERIVED from the configuration, identity mixing against the ungrouped entry point, meta
bit for bit, batch / shard independence bit for bit, the checked build, the entry point's refusals, the loader against its CPU twin
without a synchronisation, and the diversity a correlated array loses, measured by the device link on device-made frames.

The bound extends ``derived_bounds`` of tests/test_chansim_gpu.py (imported, not copied; its docstring has the ungrouped derivation and
the symbols u, M, P).  L is the float32-rounded ``mix`` the twin uses too, so the coefficients add no term.  Lambda = max_a sum_j
|L[a][j]|, n = G the largest number of sources, Gamma = M sum_p amp_p (the G of that docstring):

* a source gain z_j[p][t] is the ungrouped frame's h_p(t): its error is the ungrouped |d h_p|;
* mixing: h_a = sum_j L[a][j] z_j.  The sources' errors enter weighted, at most Lambda |d h_p|.  A term is two fused multiply-adds per
  component, each rounding a partial sum of at most Lambda amp_p M: 2 sqrt(2) n u Lambda amp_p M per tap, and every tap's phasor has
  modulus 1, so the taps together add 2 sqrt(2) n u Lambda Gamma to H;
* everything downstream (delay phasors, the sum over the taps) is the ungrouped arithmetic on gains Lambda times as large, so its error
  terms scale by Lambda:   |dH| <= Lambda channel(t_max) + 2 sqrt(2) n u Lambda Gamma;
* pilots: the same with t_max the last pilot symbol; the noise sample's own error is unchanged (the group's sigma is one of the
  table's), and the final fused multiply-add rounds a value of at most Lambda Gamma + r instead of Gamma + r.
Observed maxima are printed; DESIGN.md records them."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_conditions, simulate_frames_host
from adafortitran_amd.hip_ops import ChannelSimPlan, pack_mix
from test_chansim_gpu import _DENSE, DEV, U, _bits, _no_sync, _poison, _same_bits, _shapes, derived_bounds

pytestmark = pytest.mark.gpu
FAR = 1 << 40
FULL3 = np.array([[1.0, 0.5 + 0.3j, 0.1 - 0.2j], [0.5 - 0.3j, 1.0, 0.4 + 0.1j], [0.1 + 0.2j, 0.4 - 0.1j, 1.0]])


def derived_bounds_grouped(cfg: ChannelSimConfig):
    """(bound on |ideal - definition|, bound on |pilots - definition|) of a grouped configuration; module docstring."""
    b_ideal, b_pilots = derived_bounds(cfg)                                      # channel(T - 1), channel(last pilot symbol) + noise
    t = cfg.tables()
    r2 = np.sqrt(2.0)
    gamma = cfg.rays * float(t["tap_amp"].astype(np.float64).sum())
    r = float(t["noise_sigma"].max()) * np.sqrt(24 * np.log(2.0))
    noise_own = r * (4 * U + 4 * r2 * U)                                         # the sample's own error: unchanged
    lam = float(np.abs(t["mix"].astype(np.complex128)).sum(axis=1).max())
    mixing = 2 * r2 * cfg.group * U * lam * gamma
    channel_pilots = b_pilots - noise_own - r2 * U * (gamma + r)
    return lam * b_ideal + mixing, lam * channel_pilots + mixing + noise_own + r2 * U * (lam * gamma + r)


CONFIGS = {
    "default_2x2": (dataclasses.replace(ChannelSimConfig(), antennas=(2, 2), rx_correlation=0.7, tx_correlation=0.6 * np.exp(0.9j)), 8),
    "odd_30x7_3x1_matrix": (ChannelSimConfig(ofdm=(30, 7), pilot=(3, 1), antennas=(3, 1), rx_correlation=FULL3), 5),
    "tiles_24x40_8x2": (ChannelSimConfig(ofdm=(24, 40), pilot=(4, 4), antennas=(8, 2), rx_correlation=0.95, tx_correlation=0.95), 2),
    "dense_16": (dataclasses.replace(_DENSE, antennas=(8, 2), rx_correlation=0.8 * np.exp(-0.4j), tx_correlation=0.5), 4),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_grouped_kernel_against_the_float64_definition(name):
    cfg, groups = CONFIGS[name]
    G = cfg.group
    plan = ChannelSimPlan(cfg, DEV)
    b_ideal, b_pilots = derived_bounds_grouped(cfg)
    worst = [0.0, 0.0]
    for seed, base in ((1, 0), (2, 1 << 33)):
        batch = groups * G
        _poison(_shapes(cfg, batch))
        ideal, pilots, meta = plan(seed, base, 0, 1, FAR, batch)
        frames = base * G + np.arange(batch)
        want_i, want_p, want_m = simulate_frames_host(cfg, seed, frames)
        assert ideal.shape == want_i.shape and pilots.shape == want_p.shape and ideal.dtype == pilots.dtype == torch.complex64
        assert torch.equal(_bits(meta), _bits(torch.from_numpy(want_m)))
        got_i, got_p = ideal.cpu().numpy().astype(np.complex128), pilots.cpu().numpy().astype(np.complex128)
        assert np.isfinite(got_i).all() and np.isfinite(got_p).all()             # nothing left unwritten
        worst = [max(worst[0], float(np.abs(got_i - want_i).max())), max(worst[1], float(np.abs(got_p - want_p).max()))]
    print(f"{name}: max|ideal - def| {worst[0]:.3e} (derived bound {b_ideal:.3e})   max|pilots - def| {worst[1]:.3e} (derived bound "
          f"{b_pilots:.3e})")
    assert worst[0] <= b_ideal and worst[1] <= b_pilots


def test_identity_mixing_gives_the_ungrouped_frames():
    pinned = dict(snr_db=(10.0,), delay_spread_ns=(200.0,), doppler_hz=(800.0,))
    cfg, plain = ChannelSimConfig(antennas=(4, 2), **pinned), ChannelSimConfig(**pinned)
    assert np.array_equal(cfg.tables()["mix"], np.eye(8, dtype=np.complex64))
    for seed, base, groups in ((3, 0, 5), (4, 1 << 20, 2)):
        _poison(_shapes(cfg, 8 * groups))
        got = ChannelSimPlan(cfg, DEV)(seed, base, 0, 1, FAR, 8 * groups)
        want = ChannelSimPlan(plain, DEV)(seed, 8 * base, 0, 1, FAR, 8 * groups)
        for g, w in zip(got[:2], want[:2]):                                      # as float values: the two zeros compare equal
            assert torch.equal(torch.view_as_real(g).cpu(), torch.view_as_real(w).cpu())
        assert torch.equal(got[2].cpu(), want[2].cpu())


def test_meta_is_the_leaders_pick_bit_for_bit():
    cfg, _ = CONFIGS["dense_16"]                                                 # 16 values per condition
    G, groups, seed = 16, 24, 9
    meta = ChannelSimPlan(cfg, DEV)(seed, 7, 0, 1, FAR, G * groups)[2]
    frames = 7 * G + np.arange(G * groups)
    assert torch.equal(_bits(meta), _bits(torch.from_numpy(frame_conditions(cfg, seed, frames))))
    m = meta.cpu().view(groups, G, 3)
    assert torch.equal(m, m[:, :1].expand(groups, G, 3))                         # every member's meta is its leader's
    plain = dataclasses.replace(cfg, antennas=(1, 1), rx_correlation=None, tx_correlation=None)
    assert np.array_equal(m[:, 0].numpy(), frame_conditions(plain, seed, frames[::G]))
    assert len({tuple(r) for r in m[:, 0].tolist()}) > 12                        # ... and the groups do differ


@pytest.mark.parametrize("name", ["default_2x2", "tiles_24x40_8x2"])
def test_a_group_does_not_depend_on_its_batch_or_its_rank(name):
    cfg, _ = CONFIGS[name]
    G, groups = cfg.group, 12
    plan = ChannelSimPlan(cfg, DEV)
    _poison(_shapes(cfg, G * groups))
    whole = plan(5, 0, 0, 1, FAR, G * groups)
    by_group = [w.view(groups, G, *w.shape[1:]) for w in whole]
    for rank in range(3):                                                        # three shards of an epoch of 12 groups
        _poison(_shapes(cfg, G * 4))
        share = plan(5, 0, rank, 3, 12, G * 4)
        _same_bits(share, [w[rank::3].reshape(G * 4, *w.shape[2:]) for w in by_group])
    _poison(_shapes(cfg, G * 2))
    parts = [plan(5, 0, lo, 1, FAR, G * 2) for lo in range(0, groups, 2)]        # batches of 2 groups
    _same_bits([torch.cat([p[k] for p in parts]) for k in range(3)], whole)
    _same_bits(plan(5, 9, 0, 1, FAR, G * 3), [w[G * 9:] for w in whole])         # base counts groups
    wrapped = plan(5, 0, 10, 3, 12, G * 3)                                       # group positions 10, 13, 16 -> 10, 1, 4
    _same_bits(wrapped, [w[[10, 1, 4]].reshape(G * 3, *w.shape[2:]) for w in by_group])


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_channel_sim_group_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_channel_sim_group_f32")
    for name in ("odd_30x7_3x1_matrix", "tiles_24x40_8x2", "dense_16"):
        cfg, _ = CONFIGS[name]
        plan = ChannelSimPlan(cfg, DEV)
        batch = 3 * cfg.group
        _same_bits(plan(9, 3, 1, 2, 77, batch, lib=lib), plan(9, 3, 1, 2, 77, batch))


def test_every_refusal_of_the_entry_point_launches_nothing():
    lib = _lib.load()
    cfg = ChannelSimConfig(antennas=(2, 2), rx_correlation=0.7, tx_correlation=0.4j)
    b = 8
    outs = [torch.empty(s, dtype=dt, device=DEV) for s, dt in _shapes(cfg, b)]
    for t in outs:
        (torch.view_as_real(t) if t.is_complex() else t).fill_(float("nan"))
    ptr = [t.data_ptr() for t in outs]
    good = pack_mix(cfg.mix())
    assert good.dtype == np.float32 and good.shape == (20,)
    keep = []                                                                    # host arrays outlive their calls

    def refused(code, word, sim=None, rx=2, tx=2, mix=good, base=0, start=0, stride=1, modulo=10, batch=b, ideal=ptr[0], pilots=ptr[1],
                meta=ptr[2]):
        keep.append(mix)
        at = mix if mix is None or isinstance(mix, int) else mix.ctypes.data
        rc = lib.aft_channel_sim_group_f32(sim if sim is not None else cfg.to_struct(), rx, tx, at, 1, base, start, stride, modulo, batch,
                                           ideal, pilots, meta, None)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    rc = lib.aft_channel_sim_group_f32(None, 2, 2, good.ctypes.data, 1, 0, 0, 1, 10, b, *ptr, None)
    assert rc == E and "NULL" in lib.aft_last_error().decode()
    for k in ("ideal", "pilots", "meta", "mix"):
        refused(E, "NULL", **{k: None})
    refused(E, "8-byte", ideal=ptr[0] + 4)
    refused(E, "8-byte", pilots=ptr[1] + 4)
    refused(E, "4-byte", meta=ptr[2] + 2)
    refused(E, "4-byte", mix=good.ctypes.data + 2)
    for batch in (0, -4):
        refused(E, "batch must be at least 1", batch=batch)
    for batch in (1, 6, 7):                                                      # not a multiple of G
        refused(E, "not a multiple of rx * tx = 2 * 2", batch=batch)
    big = np.zeros(17 * 18, dtype=np.float32)
    for rx, tx, word in ((0, 2, "rx = 0"), (2, 0, "tx = 0"), (-1, -4, "rx = -1"), (17, 1, "rx = 17"), (1, 17, "tx = 17"),
                         (4, 5, "rx * tx = 20 is outside 1..16"), (16, 2, "rx * tx = 32")):
        refused(SH, word, rx=rx, tx=tx, mix=big, batch=2 * max(rx * tx, 1))
    for kw in (dict(base=-1), dict(start=-1), dict(stride=0), dict(modulo=0), dict(base=1 << 60), dict(modulo=1 << 60),
               dict(start=1 << 59, stride=1 << 59)):                             # FRAME numbers stay below 2^62: groups below 2^60 here
        refused(E, "bad frame numbers", **kw)
    for field, value, word in (("taps", 33, "taps = 33 is outside 1..32"), ("rays", 0, "rays = 0"), ("n_snr", 17, "n_snr = 17"),
                               ("n_ds", 0, "n_ds = 0"), ("n_dop", 17, "n_dop = 17"), ("pilot_scs", 65, "pilot_scs = 65"),
                               ("pilot_symbols", 17, "pilot_symbols = 17"), ("num_scs", 0, "num_scs = 0"),
                               ("num_symbols", -1, "num_symbols = -1")):
        sim = cfg.to_struct()
        setattr(sim, field, value)
        refused(SH, word, sim=sim)
    sim = cfg.to_struct()
    sim.pilot_sc_index[11] = 120
    refused(SH, "pilot_sc_index[11] = 120", sim=sim)
    for at, value in ((0, np.nan), (7, np.inf), (19, -np.inf)):
        bad = good.copy()
        bad[at] = value
        refused(E, f"mix[{at}]", mix=bad)
    torch.cuda.synchronize()
    assert all(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all() for t in outs)      # nothing was launched
    assert lib.aft_channel_sim_group_f32(cfg.to_struct(), 2, 2, good.ctypes.data, 1, 0, 0, 1, 10, b, *ptr, None) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert all(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all() for t in outs)   # ... and the good call writes it all
    _same_bits(outs, ChannelSimPlan(cfg, DEV)(1, 0, 0, 1, 10, b))
    with pytest.raises(ValueError, match="not a multiple"):
        ChannelSimPlan(cfg, DEV)(1, 0, 0, 1, 10, 6)


@pytest.mark.parametrize("fresh,drop_last", [(True, False), (False, True)])
def test_loader_on_the_device_matches_its_cpu_twin_without_a_synchronisation(fresh, drop_last):
    cfg, _ = CONFIGS["default_2x2"]
    world, G = 2, cfg.group
    b_ideal, b_pilots = derived_bounds_grouped(cfg)
    t = cfg.tables()
    lam = float(np.abs(t["mix"].astype(np.complex128)).sum(axis=1).max())
    gamma = cfg.rays * float(t["tap_amp"].astype(np.float64).sum())
    r = float(t["noise_sigma"].max()) * np.sqrt(24 * np.log(2.0))
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                                                         # the mode is honoured: the epochs below are not vacuous
    for rank in range(world):
        kw = dict(batch_size=2 * G, frames_per_epoch=9 * G, seed=4, rank=rank, world_size=world, drop_last=drop_last, fresh_each_epoch=fresh)
        dev, host = SynthLoader(cfg, device=DEV, **kw), SynthLoader(cfg, device="cpu", **kw)
        assert len(dev) == len(host)
        with _no_sync():
            epochs = [list(dev) for _ in range(2)]
        assert dev.epoch == 2
        for got in epochs:
            want = list(host)
            assert len(got) == len(want) == len(dev)
            for (pd, idv, md), (ph, ih, mh) in zip(got, want):
                assert pd.is_cuda and idv.is_cuda and not md[0].is_cuda and pd.shape == ph.shape and idv.shape == ih.shape
                assert all(torch.equal(x, y) for x, y in zip(md[:5], mh[:5])) and md[5] == mh[5]
                # the twin's batch is the definition ROUNDED to complex64: u per component of a value of at most Lambda Gamma (+ r)
                assert float((idv.cpu() - ih).abs().max()) <= b_ideal + np.sqrt(2.0) * U * lam * gamma
                assert float((pd.cpu() - ph).abs().max()) <= b_pilots + np.sqrt(2.0) * U * (lam * gamma + r)


def test_the_device_link_loses_its_diversity_to_correlation():
    """tests/test_chansim_groups.py's diversity-loss condition for R = 2, every number made on the device: frames by the grouped loader,
    bit errors by ``LinkAccumulator(branches=2)`` with perfect channel knowledge."""
    from adafortitran_amd.linksim import LinkAccumulator, LinkConfig
    errors = {}
    for rho in (None, 0.95):
        sim = ChannelSimConfig(ofdm=(24, 14), pilot=(4, 2), snr_db=(8.0,), delay_spread_ns=(200.0,), doppler_hz=(200.0,), antennas=(2, 1),
                               rx_correlation=rho)
        acc = LinkAccumulator(LinkConfig(sim, 2), DEV, seed=3, branches=2)
        for _, ideal, meta in SynthLoader(sim, 400, 1200, device=DEV, seed=3):   # 600 groups, 3 launches
            acc.update(None, ideal, meta)
        errors[rho] = acc.result() * 600 * LinkConfig(sim, 2).bits_per_frame
    print(f"R = 2 on the device: bit errors {errors[None]:.0f} at rho 0, {errors[0.95]:.0f} at rho 0.95: {errors[0.95] / errors[None]:.2f} x")
    assert errors[None] > 0 and errors[0.95] >= 1.5 * errors[None]
