"""Slot sequences in the channel simulator (adafortitran_amd/chansim.py, "time continuity") on the CPU, no library needed: K slots of a
sequence are columns of ONE long frame of the same rays (stitching), ``slots=1`` is the function it was, slot 0 is the grouped frame,
a sequence shares its leader's conditions, the sample time correlation across slots is the Bessel function of the absolute lag, every
refusal, the loader's sharding by whole sequences and the pack.

The stitching tolerance (``stitch_tolerance``).  The sequence configuration and the long single-slot configuration do the same float64
operations on the same rays except for the turn count of a ray at absolute symbol k L + t: ``rate t + frac(rate k L + phi)`` against
``rate (k L + t) + phi``.  With u = 2^-53 and A = max f_D T_sym, each side rounds products and sums of at most A K L + 1 turns at most
twice: the two turn counts differ, modulo 1, by at most u (4 A K L + 4).  A ray's exponential moves by 2 pi times that, a tap gain by
amp_p M times that, and H by Gamma = M sum_p amp_p times that; everything after the turn count is the same arithmetic on both sides,
whose own rounding (exp to an ulp, sums of P M terms of modulus at most 1) is at most 16 u Gamma.  Mixing multiplies by at most
Lambda = max_a sum_j |L[a][j]|.

The statistical bound is the one of tests/test_chansim_groups.py: sequences are independent draws, the mean over n of a per-sequence
quantity has the standard error std / sqrt(n), and every comparison must lie within 5 of them (n = 2000 as there)."""
import dataclasses

import numpy as np
import pytest

from adafortitran_amd import _abi
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_conditions, make_pack, simulate_frames_host
from test_chansim_groups import FULL3, PINNED, _todays_frames

SMALL = dict(ofdm=(6, 4), pilot=(2, 1))


def stitch_tolerance(cfg: ChannelSimConfig) -> float:
    """Bound on |sequence ideal - long frame's columns|, absolute, per complex element; module docstring."""
    t = cfg.tables()
    u = 2.0 ** -53
    A = float(t["doppler_turns"].max())
    gamma = cfg.rays * float(t["tap_amp"].astype(np.float64).sum())
    lam = float(np.abs(t["mix"].astype(np.complex128)).sum(axis=1).max())
    return lam * gamma * (2 * np.pi * u * (4 * A * cfg.slots * cfg.slot_symbols + 4) + 16 * u)


# ---- stitching ------------------------------------------------------------------------------------------------------------------

STITCH = {
    "G1": dict(ofdm=(12, 14), pilot=(3, 2), slots=3),
    "G4_complex_rho": dict(ofdm=(8, 7), pilot=(2, 1), slots=4, antennas=(2, 2), rx_correlation=0.3 + 0.6j, tx_correlation=0.5j),
    "gap_L_gt_T": dict(ofdm=(8, 5), pilot=(2, 1), slots=3, slot_symbols=9, antennas=(3, 1), rx_correlation=FULL3),
    "many_slots": dict(ofdm=(4, 14), pilot=(2, 2), slots=64, doppler_hz=(3000.0,)),
}


@pytest.mark.parametrize("name", list(STITCH))
def test_the_slots_of_a_sequence_are_columns_of_one_long_frame(name):
    kw = STITCH[name]
    cfg = ChannelSimConfig(**kw)
    K, L, G, (S, T) = cfg.slots, cfg.slot_symbols, cfg.group, cfg.ofdm
    assert L == kw.get("slot_symbols", T) and cfg.sequence() == K * G
    long = dataclasses.replace(cfg, ofdm=(S, K * L), slots=1, slot_symbols=None, pilot_symbols=None)
    seed, tol = 13, stitch_tolerance(cfg)
    seqs = np.array([0, 5, 1 << 28])
    frames = (seqs[:, None] * K * G + np.arange(K * G)[None, :]).ravel()
    got, _, got_meta = simulate_frames_host(cfg, seed, frames)
    # frame lead + a of the long configuration: its group is the sequence's first G frames (the same keys, the same conditions' leader
    # only when the long group's leader is the sequence's: pick the conditions by pinning them to the sequence's)
    worst = 0.0
    for i, q in enumerate(seqs):
        lead = q * K * G
        meta = frame_conditions(cfg, seed, [lead])[0]
        pinned = dataclasses.replace(long, snr_db=(float(meta[0]),), delay_spread_ns=(float(meta[1]),), doppler_hz=(float(meta[2]),))
        # the long configuration groups by G: frames lead .. lead + G - 1 are one of its groups, because lead is a multiple of G
        want, _, want_meta = simulate_frames_host(pinned, seed, lead + np.arange(G))
        for k in range(K):
            for a in range(G):
                mine = got[i * K * G + k * G + a]
                worst = max(worst, float(np.abs(mine - want[a][:, k * L:k * L + T]).max()))
                assert np.array_equal(got_meta[i * K * G + k * G + a], want_meta[a])
    print(f"{name}: max|slot - long frame's columns| {worst:.3e} (derived tolerance {tol:.3e})")
    assert worst <= tol
    assert tol < 1e-9                                           # the tolerance is float64 rounding, nothing wider


def test_a_sequence_shares_its_leaders_conditions():
    grid = dict(snr_db=np.linspace(-5, 40, 16), delay_spread_ns=np.linspace(10, 1000, 16), doppler_hz=np.linspace(0, 3000, 16))
    cfg = ChannelSimConfig(**SMALL, slots=3, antennas=(2, 1), rx_correlation=0.5, **grid)
    plain = ChannelSimConfig(**SMALL, **grid)
    KG, n, seed = 6, 6 * 40, 6
    frames = np.arange(n)
    want = frame_conditions(plain, seed, frames - frames % KG)                   # the sequence leader's own pick
    assert len({tuple(r) for r in want}) > 20
    assert np.array_equal(frame_conditions(cfg, seed, frames), want)
    assert np.array_equal(simulate_frames_host(cfg, seed, frames)[2], want)
    grouped = dataclasses.replace(cfg, slots=1)
    assert not np.array_equal(frame_conditions(grouped, seed, frames), want)     # the groups' own picks would have differed


# ---- slots = 1 is the function it was -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(slots=1), dict(slots=1, slot_symbols=14), dict(slots=1, slot_symbols=40),
                                dict(ofdm=(30, 7), pilot=(3, 1), slots=1)])
def test_one_slot_gives_todays_ungrouped_frames(kw):
    cfg = ChannelSimConfig(**kw)
    assert cfg.slots == 1 and cfg.sequence() == 1 and cfg.slot_symbols == kw.get("slot_symbols", cfg.ofdm[1])
    frames = np.array([0, 1, 2, 7, 1 << 33, 5])
    for got, want in zip(simulate_frames_host(cfg, 4, frames), _todays_frames(cfg, 4, frames)):
        assert got.dtype == want.dtype and np.array_equal(got, want)


def _todays_grouped(cfg: ChannelSimConfig, seed: int, frame_ids):
    """The grouped definition written out from the module docstring, on ``_todays_frames``' sources: ``mix`` row a times the ungrouped
    gains of frames lead .. lead + a at the LEADER's conditions -- what ``simulate_frames_host`` gave before the configuration had slots."""
    from adafortitran_amd.chansim import (STREAM_ANGLE, STREAM_NOISE_ANGLE, STREAM_NOISE_RADIUS, STREAM_PHASE, _conditions, frame_keys,
                                          words)
    t = cfg.tables()
    g = np.asarray(frame_ids, dtype=np.int64)
    G, (S, T), (Ps, Pt), P, M = cfg.group, cfg.ofdm, cfg.pilot, len(t["tap_delay"]), cfg.rays
    keys = frame_keys(seed, g)
    meta, (i_snr, i_ds, i_dop) = _conditions(t, frame_keys(seed, g - g % G))
    lead, where = np.unique(g - g % G, return_inverse=True)
    dop_of = np.empty(len(lead), dtype=np.int64)
    dop_of[where] = i_dop
    kk = frame_keys(seed, (lead[:, None] + np.arange(G)[None, :]).ravel())[:, None, None]
    ray = (16 * np.arange(P)[:, None] + np.arange(M)[None, :])[None]
    u = (words(kk, STREAM_ANGLE, ray) >> np.uint64(44)).astype(np.float64) * 2.0 ** -20
    phase = (words(kk, STREAM_PHASE, ray) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    rate = t["doppler_turns"].astype(np.float64)[np.repeat(dop_of, G)][:, None, None] * np.cos(2.0 * np.pi * (np.arange(M)[None, None, :] + u) / M)
    turns = rate[..., None] * np.arange(T)[None, None, None, :] + phase[..., None]
    z = (t["tap_amp"].astype(np.float64)[None, :, None] * np.exp(2j * np.pi * (turns - np.floor(turns))).sum(axis=2)).reshape(len(lead), G, P, T)
    gain = np.einsum("nj,njpt->npt", t["mix"].astype(np.complex128)[g % G], z[where])
    per_sc = t["delay_turns"].astype(np.float64)[i_ds][:, None] * t["tap_delay"].astype(np.float64)[None, :]
    x = per_sc[:, :, None] * np.arange(S)[None, None, :]
    ideal = np.einsum("nps,npt->nst", np.exp(-2j * np.pi * (x - np.floor(x))), gain)
    q = np.arange(Ps * Pt)[None, :]
    u1 = ((words(keys[:, None], STREAM_NOISE_RADIUS, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((words(keys[:, None], STREAM_NOISE_ANGLE, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23
    noise = (t["noise_sigma"].astype(np.float64)[i_snr][:, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)).reshape(len(g), Ps, Pt)
    return ideal, ideal[:, np.asarray(cfg.pilot_scs)[:, None], np.asarray(cfg.pilot_symbols)[None, :]] + noise, meta


GROUPED = [dict(antennas=(2, 2), rx_correlation=0.7, tx_correlation=0.4j), dict(ofdm=(30, 7), pilot=(3, 1), antennas=(3, 1), rx_correlation=FULL3)]


@pytest.mark.parametrize("kw", GROUPED)
def test_one_slot_gives_todays_grouped_frames(kw):
    cfg = ChannelSimConfig(slots=1, **kw)
    G = cfg.group
    frames = np.array([3 * G + 1, 0, 1, G * (1 << 30) + G - 1, 3 * G + 1, 3 * G, G - 1])
    for got, want in zip(simulate_frames_host(cfg, 4, frames), _todays_grouped(cfg, 4, frames)):
        assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("kw", GROUPED + [dict(ofdm=(12, 5), pilot=(3, 1))])
def test_slot_0_is_the_group_of_the_same_number_bit_for_bit(kw):
    K = 3
    cfg = ChannelSimConfig(slots=K, slot_symbols=kw.get("ofdm", (120, 14))[1] + 2, **PINNED, **kw)
    one = dataclasses.replace(cfg, slots=1, slot_symbols=None)
    G = cfg.group
    for q in (0, 4, 1 << 29):                                   # slot 0 of sequence q = group q K of the one-slot configuration
        frames = q * K * G + np.arange(G)
        for got, want in zip(simulate_frames_host(cfg, 8, frames), simulate_frames_host(one, 8, frames)):
            assert np.array_equal(got, want)
        later = simulate_frames_host(cfg, 8, frames + G)[0]     # ... and slot 1 is NOT the next group: the same rays, later
        assert not np.allclose(later, simulate_frames_host(one, 8, frames + G)[0])


def test_any_vector_of_frame_numbers():
    cfg = ChannelSimConfig(**SMALL, slots=3, slot_symbols=6, antennas=(2, 1), rx_correlation=0.6, **PINNED)
    whole = simulate_frames_host(cfg, 2, np.arange(24), return_noise=True)
    pick = np.array([7, 0, 23, 7, 13, 12, 5])                   # members out of order, sequences cut, a frame twice
    part = simulate_frames_host(cfg, 2, pick, return_noise=True)
    for got, all_ in zip(part, whole):
        assert np.array_equal(got, all_[pick])
    plain = dataclasses.replace(cfg, slots=1, slot_symbols=None)
    assert np.array_equal(whole[3], simulate_frames_host(plain, 2, np.arange(24), return_noise=True)[3])      # the frames' OWN noise


# ---- the time correlation across slots -----------------------------------------------------------------------------------------

def test_sample_time_correlation_across_slots_is_the_bessel_function_of_the_absolute_lag():
    theta = (np.arange(4000) + 0.5) * (np.pi / 4000)            # J0(x) = mean over theta in (0, pi) of cos(x sin theta): midpoint rule
    j0 = lambda x: np.cos(np.asarray(x)[..., None] * np.sin(theta)).mean(axis=-1)  # noqa: E731
    assert abs(j0(2.404825557695773)) < 1e-12 and abs(j0(1.0) - 0.7651976865579666) < 1e-12
    K, L, (S, T), n = 3, 6, (6, 4), 2000
    cfg = ChannelSimConfig(ofdm=(S, T), pilot=(2, 1), slots=K, slot_symbols=L, **PINNED)
    ideal = simulate_frames_host(cfg, 5, np.arange(n * K))[0].reshape(n, K, S, T)
    h = ideal.transpose(0, 2, 1, 3).reshape(n, S, K * T)                         # [n, s, (k, t)]
    per_seq = np.einsum("nsx,nsy->nxy", h, h.conj()) / S                         # subcarrier mean of H_k[s,t] conj(H_k'[s,t']), per sequence
    mean = per_seq.mean(axis=0)
    se = np.sqrt((per_seq.real.std(axis=0, ddof=1) ** 2 + per_seq.imag.std(axis=0, ddof=1) ** 2) / n)
    at = (np.arange(K)[:, None] * L + np.arange(T)[None, :]).ravel()             # the absolute symbols
    turns = float(cfg.tables()["doppler_turns"][0])
    want = j0(2 * np.pi * turns * (at[:, None] - at[None, :]))
    off = np.abs(mean - want) / np.maximum(se, 1e-300)
    off[np.diag_indices(K * T)] = 0.0
    print("worst distance in s.e.:", float(off.max()), " largest s.e.:", float(se.max()), " J0 range:", float(want.min()), float(want.max()))
    assert (se <= 0.05).all()
    assert (np.abs(mean - want) <= 5 * se + 1e-12).all()
    assert want.min() < -0.3 and abs(want[0, -1]) < 0.35                         # the lags reach past J0's first zero: not all near 1
    # independent draws per slot would have given 0 across slots: the test is not vacuous
    assert np.abs(want[:T, T:2 * T]).max() > 0.3 and np.abs(mean[:T, T:2 * T]).max() > 0.2


# ---- refusals, the loader, the pack, the signature table ----------------------------------------------------------------------

def test_refusals_of_the_configuration():
    bad = [dict(slots=0), dict(slots=-1), dict(slots=2.0), dict(slots=True), dict(slots="2"), dict(slot_symbols=13), dict(slot_symbols=0),
           dict(slots=2, slot_symbols=13), dict(slot_symbols=14.0), dict(slot_symbols=True),
           dict(slots=2, slot_symbols=2049), dict(slots=293), dict(slots=4097, ofdm=(4, 1), pilot=(1, 1)),
           dict(ofdm=(4, 2049), pilot=(1, 1), slots=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            ChannelSimConfig(**kw)
    assert _abi.AFT_CHANSIM_MAX_SLOTS == 4096 and float(np.float32(4096 * 16)) == 4096 * 16
    assert ChannelSimConfig(slots=292).sequence() == 292                         # 292 * 14 = 4088 symbols
    assert ChannelSimConfig(slots=2, slot_symbols=2048).slot_symbols == 2048
    assert ChannelSimConfig(ofdm=(4, 5000), pilot=(1, 1)).slots == 1             # one slot of any length, as before
    cfg = ChannelSimConfig(slots=4, antennas=(2, 2))
    assert cfg.sequence() == 16 and cfg.group == 4 and cfg.slot_symbols == 14
    assert dataclasses.replace(cfg, snr_db=(3.0,)).slot_symbols == 14            # a validated config validates again


def test_refusals_of_the_loader_and_the_pack():
    cfg = ChannelSimConfig(**SMALL, slots=3, antennas=(2, 1), rx_correlation=0.5)
    for kw in (dict(batch_size=4, frames_per_epoch=12), dict(batch_size=6, frames_per_epoch=16), dict(batch_size=2, frames_per_epoch=6)):
        with pytest.raises(ValueError, match="multiples of the 6 frames of slots = 3 x antennas"):
            SynthLoader(cfg, **kw)
    SynthLoader(cfg, batch_size=12, frames_per_epoch=18)
    for n in (1, 2, 4, 8):
        with pytest.raises(ValueError, match="whole sequences"):
            make_pack(cfg, n, 1)
    pack = make_pack(cfg, 12, 1)
    assert pack["h_ideal"].shape == (12, 6, 4) and pack["h_ls_sparse"].shape == (12, 6, 4) and pack["meta"].shape == (12, 5)
    assert np.array_equal(pack["meta"][:, 1:4], frame_conditions(cfg, 1, np.arange(12)))
    assert np.array_equal(pack["h_ideal"], simulate_frames_host(cfg, 1, np.arange(12))[0].astype(np.complex64))
    assert (pack["meta"][:6, 1:4] == pack["meta"][0, 1:4]).all()                 # one sequence, one set of conditions


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_shards_whole_sequences(world, drop_last):
    KG, seqs = 6, 11
    cfg = ChannelSimConfig(**SMALL, slots=3, slot_symbols=5, antennas=(2, 1), rx_correlation=0.5)
    n = KG * seqs
    for fresh in (True, False):
        ranks = [SynthLoader(cfg, 2 * KG, n, seed=2, rank=r, world_size=world, drop_last=drop_last, fresh_each_epoch=fresh)
                 for r in range(world)]
        assert len({len(ld) for ld in ranks}) == 1
        for epoch in (0, 2):
            first = epoch * n if fresh else 0
            seen = []
            for ld in ranks:
                f = ld.epoch_frames(epoch)
                assert f.dtype == np.int64 and len(f) % KG == 0
                whole = f.reshape(-1, KG)
                assert (whole[:, 0] % KG == 0).all() and (whole == whole[:, :1] + np.arange(KG)).all()     # never a split sequence
                ld.set_epoch(epoch)
                batches = list(ld)
                assert len(batches) == len(ld)
                got = np.concatenate([m[0].numpy().ravel() for _, _, m in batches]).astype(np.int64)
                assert np.array_equal(got, f)
                assert all(p.shape[0] % KG == 0 and p.shape[0] <= 2 * KG and p.shape[0] == h.shape[0] for p, h, _ in batches)
                want = simulate_frames_host(cfg, 2, f)
                assert np.array_equal(np.concatenate([h.numpy() for _, h, _ in batches]), want[0].astype(np.complex64))
                assert np.array_equal(np.concatenate([p.numpy() for p, _, _ in batches]), want[1].astype(np.complex64))
                cond = np.concatenate([np.concatenate([m[1].numpy(), m[2].numpy(), m[3].numpy()], axis=1) for _, _, m in batches])
                assert np.array_equal(cond, want[2])
                seen.append(whole[:, 0] // KG - first // KG)
            if drop_last:
                per_rank = (seqs // world) // 2 * 2
                assert all(np.array_equal(s, r + world * np.arange(per_rank)) for r, s in enumerate(seen))
            else:
                per_rank = -(-seqs // world)
                together = np.stack(seen, axis=1).ravel()
                assert np.array_equal(together, np.arange(per_rank * world) % seqs)


def test_signature_table_has_the_new_entry_points_at_abi_10():
    import ctypes as C
    assert _abi.AFT_ABI_VERSION == 10
    seq = _abi.SIGNATURES["aft_channel_sim_seq_f32"]
    group = _abi.SIGNATURES["aft_channel_sim_group_f32"]
    assert seq[0] is C.c_int and seq[1] == group[1][:4] + [C.c_int, C.c_int] + group[1][4:]     # the group's arguments plus two integers
    delayed, plain = _abi.SIGNATURES["aft_link_precoded_delayed_f32"], _abi.SIGNATURES["aft_link_precoded_f32"]
    assert delayed[0] is C.c_int and delayed[1] == plain[1][:11] + [C.c_int, C.c_int] + plain[1][11:]
    for name in ("aft_channel_sim_seq_f32", "aft_link_precoded_delayed_f32"):
        assert name in _abi.EXPORTED_SYMBOLS
    names = list(_abi.SIGNATURES)                               # each behind its sibling, the header's order
    assert names.index("aft_channel_sim_seq_f32") == names.index("aft_channel_sim_group_f32") + 1
    assert names.index("aft_link_precoded_delayed_f32") == names.index("aft_link_precoded_f32") + 1
