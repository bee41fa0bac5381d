"""Antenna correlation in the channel simulator (adafortitran_amd/chansim.py, "Kronecker frame groups") on the CPU, no library needed:
the ungrouped frames are untouched, the grouped float64 twin is ``mix @`` the ungrouped frames of the same numbers, ``mix`` is the
Kronecker product of the Cholesky factors, groups share their leader's conditions, the sample correlation of simulated groups is
``L L^H``, the LMMSE baseline's prediction holds on grouped frames unchanged, correlation costs the combiner its diversity, every
refusal, and the loader's sharding by whole groups.

The statistical bounds.  Groups are independent draws, so the mean over n groups of a per-group quantity has the standard error
std / sqrt(n) of the per-group values: the sample correlation must lie within 5 of them of ``(L L^H)[a][b]`` (16 complex comparisons; a
normal mean leaves 5 s.e. with probability 6e-7) and the LMMSE's empirical MSE within 4 of its prediction, the bound of
tests/test_lmmse.py, the s.e. taken over per-GROUP means because the members of a group are correlated."""
import dataclasses

import numpy as np
import pytest

from adafortitran_amd import _abi
from adafortitran_amd.chansim import (ChannelSimConfig, SynthLoader, _pinned, frame_conditions, frame_keys, make_pack,
                                      simulate_frames_host)

PINNED = dict(snr_db=(10.0,), delay_spread_ns=(200.0,), doppler_hz=(800.0,))
FULL3 = np.array([[1.0, 0.5 + 0.3j, 0.1 - 0.2j], [0.5 - 0.3j, 1.0, 0.4 + 0.1j], [0.1 + 0.2j, 0.4 - 0.1j, 1.0]])


def _exponential(rho, n):
    i = np.arange(n)
    d = i[:, None] - i[None, :]
    return np.where(d >= 0, complex(rho) ** np.abs(d), np.conj(complex(rho)) ** np.abs(d))


# ---- the ungrouped frames stay what they were ---------------------------------------------------------------------------------

def _todays_frames(cfg: ChannelSimConfig, seed: int, frame_ids):
    """The ungrouped definition written out once more, from the module docstring's model: what ``simulate_frames_host`` gave before
    the configuration had antennas."""
    from adafortitran_amd.chansim import (STREAM_ANGLE, STREAM_NOISE_ANGLE, STREAM_NOISE_RADIUS, STREAM_PHASE, _conditions, words)
    t = cfg.tables()
    keys = frame_keys(seed, frame_ids)
    n, (S, T), (Ps, Pt), P, M = len(keys), cfg.ofdm, cfg.pilot, len(t["tap_delay"]), cfg.rays
    meta, (i_snr, i_ds, i_dop) = _conditions(t, keys)
    kk = keys[:, None, None]
    ray = (16 * np.arange(P)[:, None] + np.arange(M)[None, :])[None]
    u = (words(kk, STREAM_ANGLE, ray) >> np.uint64(44)).astype(np.float64) * 2.0 ** -20
    phase = (words(kk, STREAM_PHASE, ray) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    rate = t["doppler_turns"].astype(np.float64)[i_dop][:, None, None] * np.cos(2.0 * np.pi * (np.arange(M)[None, None, :] + u) / M)
    turns = rate[..., None] * np.arange(T)[None, None, None, :] + phase[..., None]
    gain = t["tap_amp"].astype(np.float64)[None, :, None] * np.exp(2j * np.pi * (turns - np.floor(turns))).sum(axis=2)
    per_sc = t["delay_turns"].astype(np.float64)[i_ds][:, None] * t["tap_delay"].astype(np.float64)[None, :]
    x = per_sc[:, :, None] * np.arange(S)[None, None, :]
    ideal = np.einsum("nps,npt->nst", np.exp(-2j * np.pi * (x - np.floor(x))), gain)
    q = np.arange(Ps * Pt)[None, :]
    u1 = ((words(keys[:, None], STREAM_NOISE_RADIUS, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((words(keys[:, None], STREAM_NOISE_ANGLE, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23
    noise = (t["noise_sigma"].astype(np.float64)[i_snr][:, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)).reshape(n, Ps, Pt)
    return ideal, ideal[:, np.asarray(cfg.pilot_scs)[:, None], np.asarray(cfg.pilot_symbols)[None, :]] + noise, meta


@pytest.mark.parametrize("kw", [dict(), dict(antennas=(1, 1)), dict(antennas=(1, 1), rx_correlation=None, tx_correlation=None),
                                dict(ofdm=(30, 7), pilot=(3, 1), antennas=[1, 1])])
def test_ungrouped_configurations_give_todays_frames(kw):
    cfg = ChannelSimConfig(**kw)
    assert cfg.antennas == (1, 1) and cfg.group == 1 and cfg.rx_correlation is None and cfg.tx_correlation is None
    mix = cfg.tables()["mix"]
    assert mix.dtype == np.complex64 and mix.shape == (1, 1) and mix[0, 0] == 1
    frames = np.array([0, 1, 2, 7, 1 << 33, 5])
    for got, want in zip(simulate_frames_host(cfg, 4, frames), _todays_frames(cfg, 4, frames)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(frame_conditions(cfg, 4, frames), _todays_frames(cfg, 4, frames)[2])


# ---- mix ------------------------------------------------------------------------------------------------------------------------

def test_mix_is_the_kronecker_product_of_the_cholesky_factors():
    cases = [((2, 2), 0.7, 0.4j), ((4, 1), 0.95, None), ((1, 3), None, FULL3), ((3, 2), FULL3, 0.6 * np.exp(0.9j)), ((8, 2), 0.95, 0.95),
             ((2, 8), -0.3, 0.5 + 0.5j)]
    for antennas, rx, tx in cases:
        cfg = ChannelSimConfig(antennas=antennas, rx_correlation=rx, tx_correlation=tx)
        R, N = antennas
        G = R * N
        mix = cfg.tables()["mix"]
        assert mix.dtype == np.complex64 and mix.shape == (G, G) and cfg.group == G
        assert (mix[np.triu_indices(G, 1)] == 0).all()                           # exact zeros above the diagonal
        c = [np.eye(n) if v is None else v if isinstance(v, np.ndarray) else _exponential(v, n) for v, n in ((rx, R), (tx, N))]
        m = mix.astype(np.complex128)
        assert np.abs(m @ m.conj().T - np.kron(c[0], c[1])).max() <= 1e-6
        assert np.abs(np.diag(m @ m.conj().T) - 1).max() <= 1e-6                # every frame alone has unit power
    for antennas in ((2, 2), (8, 2), (1, 16), (16, 1), (3, 5)):
        mix = ChannelSimConfig(antennas=antennas).tables()["mix"]
        assert np.array_equal(mix, np.eye(antennas[0] * antennas[1], dtype=np.complex64))   # no correlation: the exact identity


@pytest.mark.parametrize("rho", [0.7, -0.45, 0.3 + 0.6j])                      # a complex rho among them
def test_the_exponential_model_has_a_closed_form_factor(rho):
    n = 5
    for kw, G in ((dict(antennas=(n, 1), rx_correlation=rho), n), (dict(antennas=(1, n), tx_correlation=rho), n)):
        L = ChannelSimConfig(**kw).tables()["mix"].astype(np.complex128)
        want = np.zeros((n, n), dtype=np.complex128)
        for i in range(n):
            want[i, 0] = complex(rho) ** i
            for j in range(1, i + 1):
                want[i, j] = complex(rho) ** (i - j) * np.sqrt(1 - abs(rho) ** 2)
        assert np.abs(L - want).max() <= 2.0 ** -23                              # one float32 rounding of values of at most 1


def test_a_full_matrix_is_taken_as_given():
    cfg = ChannelSimConfig(antennas=(3, 1), rx_correlation=FULL3)
    assert isinstance(cfg.rx_correlation, np.ndarray) and not cfg.rx_correlation.flags.writeable
    L = cfg.tables()["mix"].astype(np.complex128)
    assert np.abs(L - np.linalg.cholesky(FULL3)).max() <= 2.0 ** -23
    again = dataclasses.replace(cfg, snr_db=(3.0,))                              # a validated config validates again
    assert np.array_equal(again.tables()["mix"], cfg.tables()["mix"])


# ---- the grouped twin -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(antennas=(2, 2), rx_correlation=0.7, tx_correlation=0.4j),
                                dict(antennas=(3, 1), rx_correlation=FULL3, ofdm=(30, 7), pilot=(3, 1)),
                                dict(antennas=(8, 2), rx_correlation=0.95, tx_correlation=0.95, ofdm=(24, 40), pilot=(4, 4))])
def test_grouped_twin_is_mix_times_the_ungrouped_frames(kw):
    cfg = ChannelSimConfig(**PINNED, **kw)
    plain = dataclasses.replace(cfg, antennas=(1, 1), rx_correlation=None, tx_correlation=None)
    G, seed = cfg.group, 11
    L = cfg.tables()["mix"].astype(np.complex128)
    groups = np.array([0, 3, 1 << 30])
    frames = (groups[:, None] * G + np.arange(G)[None, :]).ravel()
    src_i, src_p, src_m, src_n = simulate_frames_host(plain, seed, frames, return_noise=True)
    got_i, got_p, got_m, got_n = simulate_frames_host(cfg, seed, frames, return_noise=True)
    want_i = np.einsum("ab,gbst->gast", L, src_i.reshape(len(groups), G, *cfg.ofdm)).reshape(src_i.shape)
    want_p = np.einsum("ab,gbst->gast", L, (src_p - src_n).reshape(len(groups), G, *cfg.pilot)).reshape(src_p.shape)
    assert np.abs(got_i - want_i).max() <= 1e-12 * np.abs(want_i).max()
    assert np.abs((got_p - got_n) - want_p).max() <= 1e-12 * np.abs(want_p).max()
    assert np.array_equal(got_n, src_n)                                          # the frame's OWN noise streams
    assert np.array_equal(got_m, src_m)
    # any vector of frame numbers: members out of order, groups cut, a frame twice
    pick = np.array([3 * G + 1, 0, G * (1 << 30) + G - 1, 3 * G + 1, 3 * G, G - 1])
    where = [int(np.nonzero(frames == g)[0][0]) for g in pick]
    part = simulate_frames_host(cfg, seed, pick, return_noise=True)
    for got, whole in zip(part, (got_i, got_p, got_m, got_n)):
        assert np.allclose(got, whole[where], rtol=0, atol=1e-13)


def test_every_member_has_its_leaders_conditions():
    grid = dict(snr_db=np.linspace(-5, 40, 16), delay_spread_ns=np.linspace(10, 1000, 16), doppler_hz=np.linspace(0, 3000, 16))
    cfg = ChannelSimConfig(antennas=(4, 2), rx_correlation=0.5, **grid)
    small = ChannelSimConfig(ofdm=(6, 4), pilot=(2, 1), antennas=(4, 2), rx_correlation=0.5, **grid)
    plain = ChannelSimConfig(**grid)
    G, n, seed = 8, 8 * 40, 6
    frames = np.arange(n)
    lead = frames - frames % G
    want = frame_conditions(plain, seed, lead)                                   # the leader's own pick, as an ungrouped frame
    assert len({tuple(r) for r in want}) > 20                                    # the picks do differ between groups
    assert np.array_equal(frame_conditions(cfg, seed, frames), want)
    assert np.array_equal(simulate_frames_host(small, seed, frames)[2], want)
    loader = SynthLoader(small, 16, n, seed=seed)
    meta = [m for _, _, m in loader]
    got = np.concatenate([np.concatenate([m[1].numpy(), m[2].numpy(), m[3].numpy()], axis=1) for m in meta])
    assert np.array_equal(got, want)
    assert np.array_equal(np.concatenate([m[0].numpy().ravel() for m in meta]), frames.astype(np.float32))
    pack = make_pack(small, 16, seed)
    assert np.array_equal(pack["meta"][:, 1:4], want[:16])
    # the members' own picks would have differed: the test above is not vacuous
    assert not np.array_equal(frame_conditions(plain, seed, frames), want)


def test_sample_correlation_of_simulated_groups():
    cfg = ChannelSimConfig(ofdm=(6, 4), pilot=(2, 1), antennas=(2, 2), rx_correlation=0.7, tx_correlation=0.4j, **PINNED)
    n, G = 2000, 4
    ideal = simulate_frames_host(cfg, 5, np.arange(n * G))[0].reshape(n, G, -1)
    per_group = np.einsum("nax,nbx->nab", ideal, ideal.conj()) / ideal.shape[2]      # grid mean of H_a conj(H_b), per group
    mean = per_group.mean(axis=0)
    se = np.sqrt((per_group.real.std(axis=0, ddof=1) ** 2 + per_group.imag.std(axis=0, ddof=1) ** 2) / n)
    L = cfg.tables()["mix"].astype(np.complex128)
    want = L @ L.conj().T
    print("worst distance in s.e.:", float((np.abs(mean - want) / se).max()), " largest s.e.:", float(se.max()))
    assert (se <= 0.05).all()
    assert (np.abs(mean - want) <= 5 * se).all()
    assert np.abs(want - np.kron(_exponential(0.7, 2), _exponential(0.4j, 2))).max() <= 1e-6


def test_lmmse_prediction_holds_on_grouped_frames():
    from adafortitran_amd.lmmse import LmmseTables, lmmse_estimate_host, lmmse_predicted_mse
    cond, frames, seed, G = (20, 200, 800), 1500, 7, 2                           # tests/test_lmmse.py's check, on correlated antennas
    base = ChannelSimConfig()
    cfg = _pinned(dataclasses.replace(base, antennas=(2, 1), rx_correlation=0.9), *cond)
    ideal, pilots, meta = simulate_frames_host(cfg, seed, np.arange(frames))
    assert (meta == np.asarray(cond, dtype=np.float32)).all()
    tb = LmmseTables(base)                                                       # the tables know nothing of the antennas
    per = (np.abs(lmmse_estimate_host(tb, pilots, meta) - ideal) ** 2).mean(axis=(1, 2)).reshape(frames // G, G).mean(axis=1)
    mse, se = float(per.mean()), float(per.std(ddof=1) / np.sqrt(len(per)))
    pred = lmmse_predicted_mse(tb, *cond)
    print(f"LMMSE on (2, 1) at rho 0.9: {mse:.4e}  predicted {pred:.4e}  ({(mse - pred) / se:+.2f} s.e. over {len(per)} groups)")
    assert abs(mse - pred) <= 4 * se
    # the antennas ARE correlated: the two members' channels, not only their errors
    h = ideal.reshape(frames // G, G, -1)
    assert abs((h[:, 0] * h[:, 1].conj()).mean() - 0.9) < 0.1


def _mrc_bit_errors(R: int, rho) -> int:
    from adafortitran_amd.linksim import LinkConfig, branch_weights, link_mrc_host, noise_sigma
    sim = ChannelSimConfig(ofdm=(24, 14), pilot=(4, 2), snr_db=(8.0,), delay_spread_ns=(200.0,), doppler_hz=(200.0,), antennas=(R, 1),
                           rx_correlation=rho)
    frames = np.arange(600 * R)
    ideal, _, meta = simulate_frames_host(sim, 3, frames)
    w, scale = branch_weights(meta[:, 0], 0.0, R)
    counts = link_mrc_host(LinkConfig(sim, 2), frame_keys(3, frames), ideal, ideal, noise_sigma(meta[:, 0]), w, scale, R)[0]
    return int(counts[:, 0].sum())


@pytest.mark.parametrize("R,least", [(2, 1.5), (4, 4.0)])
def test_correlation_costs_the_combiner_its_diversity(R, least):
    free, tied = _mrc_bit_errors(R, None), _mrc_bit_errors(R, 0.95)
    print(f"R = {R}: bit errors {free} at rho 0, {tied} at rho 0.95: {tied / max(free, 1):.2f} x")
    assert free > 0 and tied >= least * free


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_configuration():
    bad = [dict(antennas=(0, 1)), dict(antennas=(1, 0)), dict(antennas=(17, 1)), dict(antennas=(4, 5)), dict(antennas=(2,)),
           dict(antennas=3), dict(antennas=(2, 2, 2)),
           dict(antennas=(2, 1), rx_correlation=1.0), dict(antennas=(2, 1), rx_correlation=-1.0), dict(antennas=(2, 1), rx_correlation=1j),
           dict(antennas=(2, 1), rx_correlation=1.2), dict(antennas=(2, 1), rx_correlation=float("nan")),
           dict(antennas=(2, 1), rx_correlation=float("inf")), dict(antennas=(2, 1), rx_correlation="much"),
           dict(antennas=(2, 1), rx_correlation=[0.5, 0.5]),                              # a wrong shape
           dict(antennas=(2, 1), rx_correlation=np.eye(3)), dict(antennas=(3, 1), rx_correlation=np.ones((3, 3, 1))),
           dict(antennas=(2, 1), rx_correlation=[[1, 0.5], [0.4, 1]]),                    # not Hermitian
           dict(antennas=(2, 1), rx_correlation=[[1, 0.5j], [0.5j, 1]]),                  # symmetric, not Hermitian
           dict(antennas=(2, 1), rx_correlation=[[1, 0.5], [0.5, 1 + 1e-9]]),             # a diagonal off 1
           dict(antennas=(2, 1), rx_correlation=[[1, 1.5], [1.5, 1]]),                    # not positive definite
           dict(antennas=(2, 1), rx_correlation=[[1, 1], [1, 1]]),                        # singular
           dict(antennas=(2, 1), rx_correlation=[[1, float("nan")], [float("nan"), 1]]),
           dict(antennas=(1, 2), tx_correlation=1.0), dict(antennas=(1, 2), tx_correlation=np.eye(3)),
           dict(antennas=(1, 2), rx_correlation=0.5), dict(antennas=(2, 1), tx_correlation=0.5),    # a correlation for a dimension of 1
           dict(rx_correlation=0.3), dict(tx_correlation=[[0.9]]), dict(antennas=(1, 2), rx_correlation=[[1, 0.2], [0.2, 1]])]
    for kw in bad:
        with pytest.raises(ValueError):
            ChannelSimConfig(**kw)
    # the trivial correlation of one antenna is no correlation
    assert ChannelSimConfig(antennas=(1, 2), rx_correlation=0.0, tx_correlation=0.5).rx_correlation is None
    assert ChannelSimConfig(antennas=(1, 2), rx_correlation=[[1.0]]).rx_correlation is None
    assert ChannelSimConfig(antennas=(8, 2)).group == _abi.AFT_CHANSIM_MAX_GROUP == 16


def test_refusals_of_the_loader_and_the_pack():
    cfg = ChannelSimConfig(ofdm=(6, 4), pilot=(2, 1), antennas=(2, 2), rx_correlation=0.5)
    for kw in (dict(batch_size=6, frames_per_epoch=16), dict(batch_size=8, frames_per_epoch=18), dict(batch_size=3, frames_per_epoch=9)):
        with pytest.raises(ValueError, match="multiples of the 4 frames"):
            SynthLoader(cfg, **kw)
    SynthLoader(cfg, batch_size=8, frames_per_epoch=16)
    for n in (1, 6, 10):
        with pytest.raises(ValueError, match="whole groups"):
            make_pack(cfg, n, 1)
    with pytest.raises(ValueError, match="n >= 1"):
        make_pack(cfg, 0, 1)
    assert make_pack(cfg, 8, 1)["h_ideal"].shape == (8, 6, 4)


# ---- the loader -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_shards_whole_groups(world, drop_last):
    G, groups = 4, 11
    cfg = ChannelSimConfig(ofdm=(6, 4), pilot=(2, 1), antennas=(2, 2), rx_correlation=0.5, tx_correlation=0.3j)
    n = G * groups
    for fresh in (True, False):
        ranks = [SynthLoader(cfg, 2 * G, n, seed=2, rank=r, world_size=world, drop_last=drop_last, fresh_each_epoch=fresh)
                 for r in range(world)]
        assert len({len(ld) for ld in ranks}) == 1
        for epoch in (0, 2):
            first = epoch * n if fresh else 0
            seen = []
            for ld in ranks:
                f = ld.epoch_frames(epoch)
                assert f.dtype == np.int64 and len(f) % G == 0
                whole = f.reshape(-1, G)
                assert (whole[:, 0] % G == 0).all() and (whole == whole[:, :1] + np.arange(G)).all()       # never a split group
                ld.set_epoch(epoch)
                batches = list(ld)
                assert len(batches) == len(ld)
                got = np.concatenate([m[0].numpy().ravel() for _, _, m in batches]).astype(np.int64)
                assert np.array_equal(got, f)
                assert all(p.shape[0] % G == 0 and p.shape[0] <= 2 * G and p.shape[0] == h.shape[0] for p, h, _ in batches)
                want = simulate_frames_host(cfg, 2, f)
                assert np.array_equal(np.concatenate([h.numpy() for _, h, _ in batches]), want[0].astype(np.complex64))
                assert np.array_equal(np.concatenate([p.numpy() for p, _, _ in batches]), want[1].astype(np.complex64))
                seen.append(whole[:, 0] // G - first // G)
            if drop_last:                                       # the epoch is cut to whole rounds of ranks and whole batches: no group twice
                per_rank = (groups // world) // 2 * 2
                assert all(len(s) == per_rank for s in seen)
                together = np.concatenate(seen)
                assert len(set(together.tolist())) == len(together) and together.max() < groups
                assert all(np.array_equal(s, r + world * np.arange(per_rank)) for r, s in enumerate(seen))
            else:                                               # the ranks' groups partition the epoch, the tail wrapping as the sampler pads
                per_rank = -(-groups // world)
                assert all(len(s) == per_rank for s in seen)
                together = np.stack(seen, axis=1).ravel()                                                   # position order
                assert np.array_equal(together, np.arange(per_rank * world) % groups)
                assert set(together.tolist()) == set(range(groups))


def test_an_ungrouped_loader_is_unchanged():
    cfg = ChannelSimConfig(ofdm=(6, 4), pilot=(2, 1))
    for world, drop_last, fresh in ((1, False, True), (3, False, False), (3, True, True)):
        for rank in range(world):
            ld = SynthLoader(cfg, 4, 37, seed=1, rank=rank, world_size=world, drop_last=drop_last, fresh_each_epoch=fresh)
            m = 37 // world if drop_last else -(-37 // world)
            assert len(ld) == (m // 4 if drop_last else -(-m // 4))
            count = len(ld) * 4 if drop_last else m
            for epoch in (0, 3):
                want = (epoch * 37 if fresh else 0) + (rank + world * np.arange(count, dtype=np.int64)) % 37
                assert np.array_equal(ld.epoch_frames(epoch), want)
