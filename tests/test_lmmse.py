"""The LMMSE (Wiener) baseline's definition (adafortitran_amd/lmmse.py) on the CPU, no library needed: the Kronecker-eigenbasis form
against the direct inverse, the empirical MSE on simulated frames against the closed-form prediction (matched and mismatched), the
design-point selection rule, the constructor's refusals and J0.

The statistical bounds: the per-frame errors of n independent frames give the standard error of their mean; the empirical MSE must lie
within 4 of them of the prediction (a 6e-5 two-sided event per comparison for a normal mean; the observed distances are below 1.3)."""
import numpy as np
import pytest
import torch

from adafortitran_amd import lmmse
from adafortitran_amd.chansim import ChannelSimConfig, _pinned, ls_interpolate, simulate_frames_host
from adafortitran_amd.lmmse import LmmseEstimator, LmmseTables, lmmse_estimate_host, lmmse_predicted_mse, nearest_index

CFG = ChannelSimConfig()
SEED, FRAMES = 7, 1500
CONDITIONS = [(0, 50, 200), (20, 200, 800), (30, 50, 200), (30, 350, 1400), (10, 350, 200)]
_cache = {}


def _tables():
    if "tables" not in _cache:
        _cache["tables"] = LmmseTables(CFG)
    return _cache["tables"]


def _frames(cond):
    """(ideal, pilots, meta) of frames [0, FRAMES) of SEED drawn at one pinned condition; computed once, never written to."""
    if cond not in _cache:
        out = simulate_frames_host(_pinned(CFG, *cond), SEED, np.arange(FRAMES))
        for a in out:
            a.setflags(write=False)
        _cache[cond] = out
    return _cache[cond]


def _per_frame(est, ideal):
    return (np.abs(est - ideal) ** 2).mean(axis=(1, 2))


def _direct(tb: LmmseTables, pilots, i_snr, i_ds, i_dop):
    """kron(F, T) (R_pp + sigma2 I)^-1 p with the correlation matrices written out -- no eigen-decomposition anywhere."""
    S, T = tb.cfg.ofdm
    s, t = np.arange(S), np.arange(T)
    r_pp = np.kron(tb.r_f(tb.sc[:, None] - tb.sc[None, :], i_ds), tb.r_t(tb.sym[:, None] - tb.sym[None, :], i_dop))
    r_hp = np.kron(tb.r_f(s[:, None] - tb.sc[None, :], i_ds), tb.r_t(t[:, None] - tb.sym[None, :], i_dop))          # [ST, PsPt]
    z = np.linalg.solve(r_pp + tb.sigma2[i_snr] * np.eye(len(r_pp)), pilots.reshape(len(pilots), -1).T)
    return (r_hp @ z).T.reshape(len(pilots), S, T)


@pytest.mark.parametrize("cond", [(0, 50, 200), (20, 200, 800), (30, 50, 200)])
def test_eigenbasis_form_equals_the_direct_inverse(cond):
    tb = _tables()
    _, pilots, meta = _frames(cond)
    pilots, meta = pilots[:16], meta[:16]
    got = lmmse_estimate_host(tb, pilots, meta)
    idx = tb.indices(meta)
    assert all(len(set(i.tolist())) == 1 for i in idx)
    want = _direct(tb, pilots.astype(np.complex128), *(int(i[0]) for i in idx))
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{cond}: max|eigenbasis - direct| {err:.3e} = {err / scale:.3e} |h|max")
    assert got.dtype == np.complex128 and err <= 1e-10 * scale


@pytest.mark.parametrize("cond", CONDITIONS)
def test_empirical_mse_matches_the_prediction_and_beats_ls(cond):
    tb = _tables()
    ideal, pilots, meta = _frames(cond)
    assert (meta == np.asarray(cond, dtype=np.float32)).all()
    per = _per_frame(lmmse_estimate_host(tb, pilots, meta), ideal)
    mse, se = float(per.mean()), float(per.std(ddof=1) / np.sqrt(len(per)))
    pred = lmmse_predicted_mse(tb, *cond)
    ls = float(_per_frame(ls_interpolate(CFG, pilots).astype(np.complex128), ideal).mean())
    print(f"{cond}: LMMSE {mse:.4e}  predicted {pred:.4e}  ratio {mse / pred:.4f}  ({(mse - pred) / se:+.2f} s.e.)  LS {ls:.4e}")
    assert abs(mse - pred) <= 4 * se
    assert mse < ls
    # the pinned configuration (one value per condition) is the same design point of the full tables
    assert lmmse_predicted_mse(_pinned(CFG, *cond), *cond) == pytest.approx(pred, rel=1e-12)


def test_mismatched_design():
    tb = _tables()
    true, assume = (20, 200, 800), dict(snr_db=10, delay_spread_ns=350, doppler_hz=1400)
    ideal, pilots, meta = _frames(true)
    per = _per_frame(lmmse_estimate_host(tb, pilots, meta, assume=assume), ideal)
    matched = _per_frame(lmmse_estimate_host(tb, pilots, meta), ideal)
    mse, se = float(per.mean()), float(per.std(ddof=1) / np.sqrt(len(per)))
    pred = lmmse_predicted_mse(tb, *true, assume=assume)
    print(f"mismatched: {mse:.4e}  predicted {pred:.4e}  ({(mse - pred) / se:+.2f} s.e.)  matched {float(matched.mean()):.4e}")
    assert abs(mse - pred) <= 4 * se
    assert mse >= float(matched.mean()) and pred >= lmmse_predicted_mse(tb, *true)
    # assume at the true condition is the matched estimator, through either formula
    same = dict(snr_db=20, delay_spread_ns=200, doppler_hz=800)
    assert lmmse_predicted_mse(tb, *true, assume=same) == lmmse_predicted_mse(tb, *true)
    # the mismatched closed form, evaluated at a design that happens to be the true one, is the matched closed form
    other = lmmse_predicted_mse(tb, 10, 350, 1400, assume=None)
    assert lmmse_predicted_mse(tb, 10.2, 349, 1399, assume=assume) == other           # nearest value, both for truth and design
    # the estimate ignores the frame's meta entirely once all three are pinned
    a = lmmse_estimate_host(tb, pilots[:4], None, assume=assume)
    assert np.array_equal(a, lmmse_estimate_host(tb, pilots[:4], meta[:4], assume=assume))


def test_selection_rule():
    vals = np.asarray([0, 5, 10, 15, 20, 25, 30], dtype=np.float32)
    got = nearest_index(vals, np.asarray([-100, 0, 2.4, 2.5, 2.6, 7.5, 12.5001, 29, 1e9, np.nan, np.inf, -np.inf], dtype=np.float32))
    assert got.tolist() == [0, 0, 0, 0, 1, 1, 3, 6, 6, 0, 0, 0]           # ties to the lower index; NaN and +-inf (all distances inf) to 0
    assert nearest_index([3.0], [np.nan, 7.0]).tolist() == [0, 0]
    assert nearest_index([5.0, 1.0, 3.0], [2.0, 4.0, 0.0]).tolist() == [1, 0, 1]       # unsorted tables: first of the nearest
    tb = _tables()
    i_snr, i_ds, i_dop = tb.indices([[12.4, 120.0, 1301.0], [np.nan, 1e6, -5.0]])
    assert (i_snr.tolist(), i_ds.tolist(), i_dop.tolist()) == ([2, 0], [1, 6], [6, 0])           # 120 ns uses the 100 ns design
    assert tb.fixed(dict(delay_spread_ns=120)) == (-1, 1, -1) and tb.fixed(None) == (-1, -1, -1)
    i_snr, i_ds, i_dop = tb.indices([[12.4, 120.0, 1301.0], [np.nan, 1e6, -5.0]], assume=dict(snr_db=31, doppler_hz=0))
    assert (i_snr.tolist(), i_ds.tolist(), i_dop.tolist()) == ([6, 6], [1, 6], [0, 0])
    p = tb.to_struct(dict(snr_db=31, doppler_hz=0))
    assert (p.fixed_snr, p.fixed_ds, p.fixed_dop) == (6, -1, 0) and (p.n_snr, p.n_ds, p.n_dop) == (7, 7, 7)
    assert p.noise_var[2] == np.float32(0.1) and list(p.delay_spread_ns)[:7] == list(range(50, 351, 50))


def test_tables_and_their_image():
    cfg = ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3))
    tb = LmmseTables(cfg)
    S, T, Ps, Pt = 30, 7, 5, 3
    for lam, u, f in zip(tb.lam_f, tb.u_f, tb.f):
        assert lam.shape == (Ps,) and (lam >= 0).all() and lam.sum() == pytest.approx(Ps, rel=1e-6)     # trace of R_f: Ps sum(pw)
        assert np.allclose(u.conj().T @ u, np.eye(Ps), atol=1e-12) and f.shape == (S, Ps)
    for lam, u, t in zip(tb.lam_t, tb.u_t, tb.t):
        assert lam.shape == (Pt,) and (lam >= 0).all() and lam.sum() == pytest.approx(Pt, rel=1e-12) and t.shape == (T, Pt)
        assert u.dtype == np.float64
    img = tb.image()
    fblock, tblock = 2 * Ps * Ps + 2 * Ps * S + Ps + 1, Pt * Pt + Pt * T + Pt
    assert img.dtype == np.float32 and img.shape == (7 * fblock + 7 * tblock,)
    blk = img[3 * fblock:4 * fblock]
    ufh = blk[:2 * Ps * Ps].reshape(Ps, Ps, 2)
    assert np.array_equal(ufh[..., 0] + 1j * ufh[..., 1], tb.u_f[3].conj().T.astype(np.complex64))
    fp = blk[2 * Ps * Ps:2 * Ps * (Ps + S)].reshape(Ps, S, 2)
    assert np.array_equal(fp[..., 0] + 1j * fp[..., 1], tb.f[3].T.astype(np.complex64))
    assert np.array_equal(blk[2 * Ps * (Ps + S):-1], tb.lam_f[3].astype(np.float32)) and blk[-1] == 0
    blk = img[7 * fblock + 2 * tblock:7 * fblock + 3 * tblock]
    assert np.array_equal(blk[:Pt * Pt].reshape(Pt, Pt), tb.u_t[2].astype(np.float32))
    assert np.array_equal(blk[Pt * Pt:Pt * Pt + Pt * T].reshape(Pt, T), tb.t[2].T.astype(np.float32))
    assert np.array_equal(blk[-Pt:], tb.lam_t[2].astype(np.float32))
    # a noise-free pilot grid of a channel the model can produce is reproduced at the pilots when sigma2 -> 0: the estimator
    # interpolates.  Here: 60 dB, the estimate at the pilot positions is within 1e-3 of the pilots
    hi = LmmseTables(ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3), snr_db=(60.0,), delay_spread_ns=(50.0,), doppler_hz=(200.0,)))
    ideal, pilots, meta = simulate_frames_host(hi.cfg, 1, np.arange(8))
    est = lmmse_estimate_host(hi, pilots, meta)
    at = est[:, np.asarray(hi.cfg.pilot_scs)[:, None], np.asarray(hi.cfg.pilot_symbols)[None, :]]
    assert float(np.abs(at - pilots).max()) <= 1e-2 and float(np.abs(est - ideal).max()) <= 5e-2


def test_refusals():
    with pytest.raises(ValueError, match="ChannelSimConfig"):
        LmmseTables(dict(ofdm=(120, 14)))
    with pytest.raises(ValueError, match="ChannelSimConfig"):
        LmmseEstimator(None)
    for bad in (dict(snr=10), ["snr_db"], dict(snr_db=float("nan")), dict(doppler_hz=float("inf")), dict(delay_spread_ns=[50, 100])):
        with pytest.raises(ValueError, match="assume"):
            LmmseEstimator(CFG, assume=bad)
        with pytest.raises(ValueError, match="assume"):
            lmmse_predicted_mse(_tables(), 10, 50, 200, assume=bad)
    tb = _tables()
    pilots = np.zeros((3, 12, 2), np.complex64)
    with pytest.raises(ValueError, match="pilot shape"):
        lmmse_estimate_host(tb, np.zeros((3, 2, 12), np.complex64), np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        lmmse_estimate_host(tb, pilots, np.zeros((3, 2)))
    with pytest.raises(ValueError, match="3 frames but 2 rows"):
        lmmse_estimate_host(tb, pilots, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="conditions are required"):
        lmmse_estimate_host(tb, pilots, None, assume=dict(snr_db=10))
    model = LmmseEstimator(CFG)
    meta = tuple(torch.zeros(3, 1) for _ in range(5)) + ([("SYNTH",) * 3],)
    with pytest.raises(ValueError, match="pilot shape"):
        model(torch.zeros(3, 2, 12, dtype=torch.complex64), meta)
    with pytest.raises(ValueError, match="complex64"):
        model(torch.zeros(3, 12, 2, dtype=torch.complex128), meta)
    with pytest.raises(ValueError, match="meta_data is required"):
        model(torch.zeros(3, 12, 2, dtype=torch.complex64))
    with pytest.raises(ValueError, match="one value per frame"):
        model(torch.zeros(4, 12, 2, dtype=torch.complex64), meta)
    with pytest.raises(ValueError, match="too few"):
        lmmse.j0(600.0, n=512)


def test_module_on_the_cpu_is_the_definition_rounded():
    import adafortitran_amd
    from adafortitran_amd import chansim, evaluation, ingest
    assert adafortitran_amd.LmmseEstimator is LmmseEstimator
    model = LmmseEstimator(CFG)
    assert list(model.parameters()) == [] and [n for n, _ in model.named_buffers()] == ["table_image"] and model.state_dict() == {}
    assert model.table_image.dtype == torch.float32 and np.array_equal(model.table_image.numpy(), _tables().image())
    loader = chansim.SynthLoader(CFG, 8, 16, device="cpu", seed=3)
    for pilots, ideal, meta in loader:
        got = model(pilots, meta)
        cond = np.concatenate([m.numpy() for m in meta[1:4]], axis=1)
        want = lmmse_estimate_host(_tables(), pilots.numpy(), cond).astype(np.complex64)
        assert got.dtype == torch.complex64 and got.shape == ideal.shape and np.array_equal(got.numpy(), want)
    pinned = LmmseEstimator(CFG, assume=dict(snr_db=10, delay_spread_ns=100, doppler_hz=400))
    assert pinned.fixed == (2, 1, 1) and pinned(pilots).shape == ideal.shape                       # no meta needed
    # the evaluation sweep measures it like any estimator: a module without parameters, its device found from its buffer
    packs = [(f"SNR_{snr}", ingest.ResidentLoader(chansim.make_pack(CFG, 32, seed=5, snr_db=snr), CFG.pilot, 16, device="cpu",
                                                   shuffle=False)) for snr in (20, 0)]
    stats = evaluation.get_test_stats(model, packs)
    assert list(stats) == [0, 20] and stats[20] < stats[0] < 0
    pack = chansim.make_pack(CFG, 32, seed=5, snr_db=0)
    sc, sym = np.asarray(CFG.pilot_scs), np.asarray(CFG.pilot_symbols)
    pil = pack["h_ls_sparse"][:, sc[:, None], sym[None, :]]
    want = lmmse_estimate_host(_tables(), pil, pack["meta"][:, 1:4]).astype(np.complex64)
    mse = float((np.abs(want.astype(np.complex128) - pack["h_ideal"]) ** 2).mean())
    assert stats[0] == pytest.approx(10 * np.log10(mse), abs=1e-9)


def test_j0_against_known_values():
    known = {0.0: 1.0, 1.0: 0.7651976865579666, 2.404825557695773: 0.0, 5.0: -0.1775967713143383, 5.520078110286311: 0.0,
             10.0: -0.2459357644513483, 30.0: -0.0863679835810403, 60.0: -0.0914718040890620}
    x = np.asarray(list(known))
    got = lmmse.j0(x)
    print("J0 errors", np.abs(got - np.asarray(list(known.values()))))
    assert np.abs(got - np.asarray(list(known.values()))).max() <= 2e-15
    assert np.array_equal(lmmse.j0(-x), got) and lmmse.j0(x.reshape(2, 4)).shape == (2, 4)
    assert abs(float(lmmse.j0(1000.0)) - 0.02478668615242) <= 1e-13                   # N grows with the argument
