"""Choosing the LMMSE design point from the pilots: the float64 twin ``lmmse.lmmse_classify_host`` against the brute-force Gaussian
log-likelihood, its rules (ties, NaN, ``assume``, empty windows, pooling), its invariances, its refusals, what it is worth (blind NMSE
against genie and robust on the float64 twins), and the CPU paths of ``ConditionEstimator``, ``LmmseEstimator(conditions="estimated")``
and ``EstimatedConditions``.  No GPU, no library."""
import dataclasses

import numpy as np
import pytest
import torch

from adafortitran_amd import lmmse
from adafortitran_amd.chansim import ChannelSimConfig, simulate_frames_host
from adafortitran_amd.lmmse import (ConditionEstimator, EstimatedConditions, LmmseEstimator, LmmseTables, lmmse_classify_host,
                                    lmmse_estimate_host, lmmse_seq_estimate_host)

SMALL = ChannelSimConfig(ofdm=(24, 6), pilot=(5, 2), slots=4, slot_symbols=6)
GROUPED = dataclasses.replace(SMALL, antennas=(2, 1))
_cache = {}


def _small():
    """(tables W = 3 h = 1, pilots of two sequences, idx, values, scores), made once."""
    if "small" not in _cache:
        tb = LmmseTables(SMALL, 3, 1)
        _, pilots, _ = simulate_frames_host(SMALL, 11, np.arange(2 * SMALL.sequence()))
        out = lmmse_classify_host(tb, pilots, return_scores=True)
        for a in (pilots, *out):
            a.setflags(write=False)
        _cache["small"] = (tb, pilots, *out)
    return _cache["small"]


def _flat(idx, sizes=(7, 7, 7)):
    return (idx[:, 0] * sizes[1] + idx[:, 1]) * sizes[2] + idx[:, 2]


def test_scores_are_the_gaussian_log_likelihood():
    """-(log det C + p^H C^-1 p), C = R_f (x) R_t^(w) + sigma2 I from ``tables.r_f`` / ``r_t``, for every candidate: 1e-9 relative.
    The eigenvalues the tables clamp at 0 are dropped from neither side (both keep all Ps w Pt terms) and the comparison holds with
    them in."""
    tb, pilots, idx, values, scores = _small()
    K = SMALL.slots
    assert scores.shape == (len(pilots), 343) and idx.shape == values.shape == (len(pilots), 3)
    assert idx.dtype == np.int64 and values.dtype == np.float32
    worst = 0.0
    for f in range(len(pilots)):
        w = int(tb.slot_window(f % K))
        if w == 0:
            continue
        p = np.concatenate([pilots[f - (tb.horizon + w - 1 - i)] for i in range(w)], axis=1).reshape(-1)
        q = tb.window_symbols(w)
        for d in range(7):
            r_f = tb.r_f(tb.sc[:, None] - tb.sc[None, :], d)
            for e in range(7):
                r = np.kron(r_f, tb.r_t(q[:, None] - q[None, :], e))
                for s in range(7):
                    c = r + tb.sigma2[s] * np.eye(len(p))
                    want = -(np.linalg.slogdet(c)[1] + np.real(p.conj() @ np.linalg.solve(c, p)))
                    got = scores[f, (s * 7 + d) * 7 + e]
                    worst = max(worst, abs(got - want) / abs(want))
    print(f"largest relative difference to the brute-force log-likelihood: {worst:.3e}")
    assert worst <= 1e-9
    assert np.array_equal(_flat(idx), scores.argmax(axis=1))
    for k, name in enumerate(lmmse.CONDITIONS):
        assert np.array_equal(values[:, k], tb.values[name][idx[:, k]].astype(np.float32))


def test_empty_windows_choose_index_zero_with_score_zero():
    tb, pilots, idx, values, scores = _small()
    first = np.arange(len(pilots)) % SMALL.slots == 0                  # h = 1: slot 0 has nothing to look at
    assert not idx[first].any() and not scores[first].any() and scores[~first].all()
    nan = np.array(pilots)
    nan[first] = np.nan                                                # ... and is not read by anybody's window but slot 1 .. 3's
    idx2, _ = lmmse_classify_host(tb, nan)
    assert not idx2.any()
    pinned, _, sc = lmmse_classify_host(tb, pilots, assume=dict(doppler_hz=1400), return_scores=True)
    assert (pinned[first] == [0, 0, 6]).all()
    assert np.array_equal(sc[first][0] == 0, np.arange(343) % 7 == 6) and np.isneginf(sc[first][0][np.arange(343) % 7 != 6]).all()


def test_ties_go_to_the_lowest_flat_index():
    """Constructed equal scores: two delay spreads and two Dopplers with the SAME value have the same tables, so their candidates tie
    exactly."""
    cfg = ChannelSimConfig(ofdm=(24, 6), pilot=(5, 2), delay_spread_ns=(300.0, 50.0, 300.0), doppler_hz=(900.0, 900.0, 100.0),
                           snr_db=(20.0, 0.0))
    tb = LmmseTables(cfg)
    _, pilots, _ = simulate_frames_host(cfg, 3, np.arange(64))
    idx, _, sc = lmmse_classify_host(tb, pilots, return_scores=True)
    sc = sc.reshape(64, 2, 3, 3)
    assert np.array_equal(sc[:, :, 0], sc[:, :, 2]) and np.array_equal(sc[:, :, :, 0], sc[:, :, :, 1])
    assert (idx[:, 1] != 2).all() and (idx[:, 2] != 1).all() and len(np.unique(idx, axis=0)) > 2
    flat = sc.reshape(64, -1)
    twinned = (idx[:, 1] == 0) | (idx[:, 2] == 0)                                              # a winner at a doubled value has an exact twin ...
    assert twinned.sum() >= 16 and ((flat == flat.max(axis=1, keepdims=True)).sum(axis=1)[twinned] >= 2).all()
    assert np.array_equal(_flat(idx, (2, 3, 3)), [int(np.flatnonzero(r == r.max())[0]) for r in flat])   # ... and the lower one is chosen


def test_nan_pilots_never_win():
    tb = LmmseTables(ChannelSimConfig())
    _, pilots, _ = simulate_frames_host(tb.cfg, 5, np.arange(4))
    want, _ = lmmse_classify_host(tb, pilots)
    bad = np.array(pilots)
    bad[1, 3, 1] = np.nan
    idx, values, sc = lmmse_classify_host(tb, bad, return_scores=True)
    assert np.isnan(sc[1]).all() and not idx[1].any() and np.array_equal(idx[[0, 2, 3]], want[[0, 2, 3]])
    assert np.array_equal(values[1], [tb.values[k][0] for k in lmmse.CONDITIONS])
    idx, _ = lmmse_classify_host(tb, bad, assume=dict(snr_db=30, doppler_hz=0))
    assert (idx[1] == [6, 0, 0]).all()                                  # the pinned index, 0 where free


def test_assume_pins_one_two_and_three_conditions():
    tb, pilots, idx, _, scores = _small()
    live = np.arange(len(pilots)) % SMALL.slots != 0
    cube = scores.reshape(-1, 7, 7, 7)
    one, _, s1 = lmmse_classify_host(tb, pilots, assume=dict(delay_spread_ns=210.0), return_scores=True)   # nearest value: 200 ns, index 3
    fixed = tb.fixed(dict(delay_spread_ns=210.0))
    assert fixed[0] == -1 and fixed[2] == -1 and (one[:, 1] == fixed[1]).all()
    d = fixed[1]
    s1 = s1.reshape(-1, 7, 7, 7)
    assert np.array_equal(s1[:, :, d], cube[:, :, d]) and np.isneginf(np.delete(s1, d, axis=2)).all()
    assert np.array_equal((one[:, 0] * 7 + one[:, 2])[live], cube[live][:, :, d].reshape(-1, 49).argmax(axis=1))
    two, _ = lmmse_classify_host(tb, pilots, assume=dict(snr_db=20, doppler_hz=1400))
    assert (two[:, 0] == 4).all() and (two[:, 2] == 6).all()
    assert np.array_equal(two[live, 1], cube[live][:, 4, :, 6].argmax(axis=1))
    three, vals, s3 = lmmse_classify_host(tb, np.full_like(pilots, np.nan), assume=dict(snr_db=20, delay_spread_ns=350, doppler_hz=1400),
                                          return_scores=True)           # nothing is computed: the pilots are not looked at
    assert (three == [4, 6, 6]).all() and (vals == [20, 350, 1400]).all()
    assert (s3[:, (4 * 7 + 6) * 7 + 6] == 0).all() and np.isneginf(s3).sum() == 342 * len(pilots)


def test_a_frame_that_decides_alone_and_a_group_that_decides_together():
    tb = LmmseTables(GROUPED, 3, 1)
    _, pilots, _ = simulate_frames_host(GROUPED, 11, np.arange(3 * GROUPED.sequence()))
    alone = lmmse_classify_host(tb, pilots, pool=False, return_scores=True)
    assert alone[2].shape == (len(pilots), 343)
    for a in range(2):                                                  # member a's frames, classified as sequences of G = 1
        single = lmmse_classify_host(LmmseTables(SMALL, 3, 1), pilots[a::2], return_scores=True)
        assert all(np.array_equal(x[a::2], y) for x, y in zip(alone, single))
    idx, _, pooled = lmmse_classify_host(tb, pilots, return_scores=True)
    assert pooled.shape == (len(pilots) // 2, 343) and np.array_equal(idx[0::2], idx[1::2])
    full = np.arange(len(pooled)) % 4 == 3                              # E adds over the members, the log-determinant counts twice
    assert np.allclose(pooled[full], alone[2][0::2][full] + alone[2][1::2][full], rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="pool must be True"):
        lmmse_classify_host(tb, pilots, pool=1)


def test_a_window_cut_out_of_a_longer_sequence_gives_the_same_choice():
    cfg = ChannelSimConfig(slots=6)
    _, pilots, _ = simulate_frames_host(cfg, 9, np.arange(12))
    W = 3
    idx, _, sc = lmmse_classify_host(LmmseTables(cfg, W, 0), pilots, return_scores=True)
    short = LmmseTables(dataclasses.replace(cfg, slots=W), W, 0)
    for k in range(W - 1, 6):
        cut_idx, _, cut = lmmse_classify_host(short, pilots[k - W + 1:k + 1], return_scores=True)
        assert np.array_equal(cut_idx[-1], idx[k]) and np.array_equal(cut[-1], sc[k])


def test_single_slot_twin_on_a_bare_config_is_the_sequence_twin_with_one_slot():
    cfg = ChannelSimConfig()
    _, pilots, _ = simulate_frames_host(cfg, 4, np.arange(37))          # any batch
    bare = lmmse_classify_host(cfg, pilots, return_scores=True)
    tabled = lmmse_classify_host(LmmseTables(cfg, 1, 0), pilots, return_scores=True)
    seq = lmmse_classify_host(LmmseTables(ChannelSimConfig(slots=37), 1, 0), pilots, return_scores=True)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(bare, tabled, seq))
    tb = LmmseTables(cfg)
    assert tb.classify_image().dtype == np.float32 and tb.classify_image().shape == (7 * 7 * 1 * 7,)
    tb4 = LmmseTables(ChannelSimConfig(slots=4), 4, 0)
    img = tb4.classify_image().reshape(7, 7, 4, 7)
    assert np.array_equal(img[:, :, 0].reshape(-1), tb.classify_image())                       # w = 1 is the single-slot table
    assert np.array_equal(img[2, 5, 2], tb4.logdet(2, 5, 3).astype(np.float32))
    v = tb4.lam_f[2][:, None] * tb4.time(5, 3)[0][None, :] + tb4.sigma2[4]
    assert abs(tb4.logdet(2, 5, 3)[4] - np.log(v).sum()) <= 1e-12 * abs(np.log(v).sum())


def test_image_and_seq_image_are_untouched():
    """The new table is a table of its own: the two images keep their lengths (the header's layout) and their content."""
    tb = LmmseTables(ChannelSimConfig(slots=4), 3, 1)
    fblocks = 7 * (2 * 144 + 2 * 12 * 120 + 12)
    assert tb.image().shape == (fblocks + 7 * (4 + 2 * 14 + 2),)
    assert tb.seq_image().shape == (fblocks + 7 * sum(2 * w * (2 * w + 14 + 1) for w in (1, 2, 3)),)
    assert np.array_equal(tb.image(), LmmseTables(ChannelSimConfig()).image())
    assert np.array_equal(tb.seq_image()[:fblocks], tb.image()[:fblocks])


def test_refusals_name_the_fix():
    tb = LmmseTables(GROUPED, 3, 1)
    _, pilots, _ = simulate_frames_host(GROUPED, 1, np.arange(GROUPED.sequence()))
    with pytest.raises(ValueError, match=r"not whole sequences: pass a multiple of slots \* group = 4 \* 2 = 8"):
        lmmse_classify_host(tb, pilots[:6])
    with pytest.raises(ValueError, match=r"not whole sequences"):
        lmmse_classify_host(tb, pilots[:6], pool=False)
    with pytest.raises(ValueError, match=r"not whole groups: pass a multiple of group = 2 frames.*pool=False"):
        lmmse_classify_host(GROUPED, pilots[:3])
    assert len(lmmse_classify_host(GROUPED, pilots[:3], pool=False)[0]) == 3
    with pytest.raises(ValueError, match="Expected pilot shape"):
        lmmse_classify_host(tb, pilots[:, :4])
    with pytest.raises(ValueError, match="assume must be a dict with keys from"):
        lmmse_classify_host(tb, pilots, assume=dict(snr=3))
    with pytest.raises(ValueError, match="need a slot sequence"):
        ConditionEstimator(ChannelSimConfig(), window=2)
    with pytest.raises(ValueError, match='choose "meta"'):
        LmmseEstimator(ChannelSimConfig(), conditions="blind")
    with pytest.raises(ValueError, match="pool must be True"):
        ConditionEstimator(ChannelSimConfig(), pool="yes")
    with pytest.raises(ValueError, match="complex64"):
        ConditionEstimator(ChannelSimConfig())(torch.zeros(2, 12, 2))
    with pytest.raises(ValueError, match="wraps an nn.Module"):
        EstimatedConditions(lambda p, m: p, ChannelSimConfig())


def _nmse(est, ideal):
    return float((np.abs(est - ideal) ** 2).sum() / (np.abs(ideal) ** 2).sum())


def _three_nmse(cfg, W, frames, pool=True):
    """(genie, blind, robust) NMSE over the steady slots, all conditions, on the float64 twins; robust = ``assume`` at the grid's highest
    SNR, delay spread and Doppler."""
    tb = LmmseTables(cfg, W, 0)
    ideal, pilots, meta = simulate_frames_host(cfg, 7, np.arange(frames))
    host = lmmse_seq_estimate_host if tb.multi_slot else lmmse_estimate_host
    top = {k: float(tb.values[k].max()) for k in lmmse.CONDITIONS}
    blind = lmmse_classify_host(tb, pilots, pool=pool)[1]
    steady = np.arange(frames) // cfg.group % cfg.slots >= W - 1
    out = [_nmse(host(tb, pilots, c, a)[steady], ideal[steady]) for c, a in ((meta, None), (blind, None), (meta, top))]
    hit = [float((lmmse.nearest_index(tb.values[k], meta[:, i]) == lmmse.nearest_index(tb.values[k], blind[:, i]))[steady].mean())
           for i, k in enumerate(lmmse.CONDITIONS)]
    return out, hit


def test_blind_single_slot_beats_the_mean_of_genie_and_robust():
    (genie, blind, robust), hit = _three_nmse(ChannelSimConfig(), 1, 512)
    print(f"slots = 1, 512 frames: NMSE genie {genie:.4f}  blind {blind:.4f}  robust {robust:.4f}   hit rate snr / ds / dop "
          f"{hit[0]:.2f} / {hit[1]:.2f} / {hit[2]:.2f}")
    assert genie < blind < 0.5 * (genie + robust)


def test_blind_pooled_window_beats_the_mean_of_genie_and_robust():
    cfg = ChannelSimConfig(slots=8, antennas=(4, 1))
    (genie, blind, robust), hit = _three_nmse(cfg, 4, 16 * cfg.sequence())
    print(f"slots = 8, W = 4, antennas = (4, 1), 16 sequences: NMSE genie {genie:.4f}  blind {blind:.4f}  robust {robust:.4f}   hit rate "
          f"snr / ds / dop {hit[0]:.2f} / {hit[1]:.2f} / {hit[2]:.2f}")
    assert genie < blind < 0.5 * (genie + robust)


def test_modules_on_the_cpu_are_the_twin():
    cfg = GROUPED
    tb = LmmseTables(cfg, 3, 1)
    ideal, pilots, meta = simulate_frames_host(cfg, 21, np.arange(2 * cfg.sequence()))
    pil = torch.from_numpy(pilots.astype(np.complex64))
    p32 = pil.numpy()
    for assume, pool in ((None, True), (dict(snr_db=10), True), (None, False)):
        want_idx, want_val, want_sc = lmmse_classify_host(tb, p32, assume, pool, return_scores=True)
        chooser = ConditionEstimator(cfg, 3, 1, assume=assume, pool=pool)
        assert list(chooser.parameters()) == [] and chooser.table_image.dtype == chooser.logdet_image.dtype == torch.float32
        assert np.array_equal(chooser.logdet_image.numpy(), tb.classify_image())
        snr, ds, dop = chooser(pil)
        assert all(c.dtype == torch.float32 and c.shape == (len(pil),) for c in (snr, ds, dop))
        assert np.array_equal(torch.stack([snr, ds, dop], dim=1).numpy(), want_val)
        idx, *_, sc = chooser.classify(pil, scores=True)
        assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(sc.numpy(), want_sc)
        # the blind baseline: the twin's estimate at the chosen conditions, whatever the meta says
        model = LmmseEstimator(cfg, assume=assume, window=3, horizon=1, conditions="estimated", pool=pool)
        want = lmmse_seq_estimate_host(tb, p32, want_val, assume).astype(np.complex64)
        junk = (None, torch.full((len(pil), 1), float("nan")), torch.zeros(len(pil), 1), torch.zeros(len(pil), 1), None, None)
        assert np.array_equal(model(pil, None).numpy(), want) and np.array_equal(model(pil, junk).numpy(), want)
        assert model.get_model_info()["conditions"] == "estimated"
        # the wrapper: a hand-made substitution into the six-tuple
        given = tuple(torch.from_numpy(np.ascontiguousarray(meta[:, k:k + 1])) for k in range(3))
        six = (torch.arange(len(pil)), *given, 8, ["a"])
        seen = {}

        class Spy(torch.nn.Module):
            def forward(self, pilot_symbols, meta_data):
                seen["meta"] = meta_data
                return LmmseEstimator(cfg, assume=assume, window=3, horizon=1)(pilot_symbols, meta_data)

        wrapped = EstimatedConditions(Spy(), cfg, window=3, horizon=1, assume=assume, pool=pool)
        got = wrapped(pil, six)
        by_hand = (six[0], *(torch.from_numpy(np.ascontiguousarray(want_val[:, k:k + 1])) for k in range(3)), 8, ["a"])
        assert seen["meta"][0] is six[0] and seen["meta"][4] == 8 and seen["meta"][5] is six[5]
        assert all(torch.equal(a, b) and a.shape == (len(pil), 1) for a, b in zip(seen["meta"][1:4], by_hand[1:4]))
        assert np.array_equal(got.numpy(), LmmseEstimator(cfg, assume=assume, window=3, horizon=1)(pil, by_hand).numpy())
        assert np.array_equal(got.numpy(), want)
        assert np.array_equal(wrapped(pil).numpy(), want) and seen["meta"][0] is None and seen["meta"][1].shape == (len(pil), 1)
    assert model.table_image is model.chooser.table_image and model.double().float().table_image is model.chooser.table_image
    default = LmmseEstimator(cfg, window=3, horizon=1)
    assert default.conditions == "meta" and default.chooser is None
    with pytest.raises(ValueError, match="meta_data is required"):
        default(pil, None)


def test_evaluation_sweep_measures_a_blind_estimator_unchanged():
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import make_pack
    from adafortitran_amd.evaluation import get_test_stats
    cfg = ChannelSimConfig()
    packs = {snr: make_pack(cfg, 64, seed=30 + snr, snr_db=snr) for snr in (0, 20)}

    def loaders():
        return [(f"SNR_{snr}", ingest.ResidentLoader(pack, cfg.pilot, 32, device="cpu", shuffle=False)) for snr, pack in packs.items()]

    genie = get_test_stats(LmmseEstimator(cfg), loaders())
    blind = get_test_stats(LmmseEstimator(cfg, conditions="estimated"), loaders())
    wrapped = get_test_stats(EstimatedConditions(LmmseEstimator(cfg), cfg), loaders())
    robust = get_test_stats(LmmseEstimator(cfg, assume=dict(snr_db=30, delay_spread_ns=350, doppler_hz=1400)), loaders())
    print(f"MSE in dB per SNR: genie {genie}  blind {blind}  robust {robust}")
    assert blind == wrapped and list(blind) == [0, 20]
    assert all(genie[k] <= blind[k] for k in blind) and blind[0] < robust[0]
