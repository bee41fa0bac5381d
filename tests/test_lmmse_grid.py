"""The full-grid smoother's definition (``lmmse.lmmse_grid_host``, ``LmmseTables.grid()``, ``lmmse_grid_predicted_mse``) on the CPU, no
library needed: on an all-pilot configuration it IS the pilot estimator; building its tables leaves the three images the existing
kernels read byte for byte; its exact MSE with the sent symbols known against Monte Carlo; its refusals.

The statistical bound is tests/test_lmmse.py's: the per-frame errors of n independent frames give the standard error of their mean,
and the empirical MSE must lie within 4 of them of the prediction."""
import numpy as np
import pytest

from adafortitran_amd import _abi
from adafortitran_amd.chansim import ChannelSimConfig, _pinned, frame_keys, simulate_frames_host
from adafortitran_amd.linksim import LinkConfig, data_noise_scale, link_observe_host, noise_sigma
from adafortitran_amd.lmmse import (GridTables, LmmseTables, lmmse_estimate_host, lmmse_grid_host, lmmse_grid_predicted_mse,
                                    lmmse_predicted_mse)

CFG = ChannelSimConfig()
SEED, FRAMES = 7, 200


@pytest.mark.parametrize("shape", [(30, 7), (3, 5)])
def test_on_an_all_pilot_grid_the_smoother_is_the_pilot_estimator(shape):
    """``pilot = (S, T)``: every position is a pilot, so both definitions are the same linear map.  30 x 7 keeps Kf = 12 of 30
    eigen-directions (the dropped eigenvalues are rounding), 3 x 5 has Kf = S = 3 < taps."""
    cfg = ChannelSimConfig(ofdm=shape, pilot=shape)
    tb = LmmseTables(cfg)
    _, pilots, meta = simulate_frames_host(cfg, 5, np.arange(12))
    want, got = lmmse_estimate_host(tb, pilots, meta), lmmse_grid_host(tb, pilots, meta)
    g = tb.grid()
    assert g.kf == min(shape[0], 12) and all(lam.shape == (g.kf,) and (np.diff(lam) <= 0).all() and (lam >= 0).all() for lam in g.lam_g)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{shape}: max|grid - pilot estimator| {err:.3e} = {err / scale:.3e} |est|max")
    assert got.dtype == np.complex128 and err <= 1e-10 * scale
    # the pinned receiver picks the same design point for every frame
    pinned = dict(snr_db=20.0, delay_spread_ns=200.0, doppler_hz=800.0)
    a, b = lmmse_estimate_host(tb, pilots, None, assume=pinned), lmmse_grid_host(tb, pilots, None, assume=pinned)
    assert float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(a).max())


def test_building_the_grid_tables_leaves_the_three_images_byte_for_byte():
    seq = ChannelSimConfig(slots=4)
    for cfg, kw in ((CFG, {}), (ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3)), {}), (seq, dict(window=2, horizon=1))):
        tb, fresh = LmmseTables(cfg, **kw), LmmseTables(cfg, **kw)
        before = [tb.image().tobytes(), tb.seq_image().tobytes(), tb.classify_image().tobytes()]
        g = tb.grid()
        assert isinstance(g, GridTables) and tb.grid() is g                      # built once
        after = [tb.image().tobytes(), tb.seq_image().tobytes(), tb.classify_image().tobytes()]
        assert before == after == [fresh.image().tobytes(), fresh.seq_image().tobytes(), fresh.classify_image().tobytes()]
        S, T = cfg.ofdm
        n_ds, n_dop = len(tb.delay_turns), len(tb.doppler_turns)
        img = g.image()
        assert img.dtype == np.float32 and img.size == n_ds * (4 * S * g.kf + g.kf + (g.kf & 1)) + n_dop * (2 * T * T + T)
        # the first block: U_g^H s-major, then F_g k-major, then the eigenvalues
        ugh = img[:2 * S * g.kf].reshape(S, g.kf, 2)
        assert np.allclose(ugh[..., 0] + 1j * ugh[..., 1], g.u_g[0].conj(), atol=1e-7)
        fg = img[2 * S * g.kf:4 * S * g.kf].reshape(g.kf, S, 2)
        assert np.allclose(fg[..., 0] + 1j * fg[..., 1], (g.u_g[0] * g.lam_g[0]).T, atol=1e-5)
        assert np.allclose(img[4 * S * g.kf:4 * S * g.kf + g.kf], g.lam_g[0], rtol=1e-6, atol=1e-30)


@pytest.mark.parametrize("cond", [(20, 200, 800), (10, 350, 200)])
def test_predicted_mse_with_the_sent_symbols_known_against_monte_carlo(cond):
    """16-QAM: the noise of z is sigma2 / |x|^2 at a data element, 17/9 sigma2 on average, and sigma2 at a pilot."""
    m = 4
    sim = _pinned(CFG, *cond)
    tb = LmmseTables(CFG)
    ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(FRAMES))
    keys, sigma = frame_keys(SEED, np.arange(FRAMES)), noise_sigma(meta[:, 0])
    z, decisions, _ = link_observe_host(LinkConfig(sim, m), keys, ideal, ideal, sigma, np.ones(FRAMES, dtype=np.float32), pilots,
                                        source="sent")
    est = lmmse_grid_host(tb, z, meta, noise_scale=data_noise_scale(m))
    per = (np.abs(est - ideal) ** 2).mean(axis=(1, 2))
    mse, se = float(per.mean()), float(per.std(ddof=1) / np.sqrt(len(per)))
    pred = lmmse_grid_predicted_mse(tb, *cond, m)
    pilot_only = lmmse_predicted_mse(tb, *cond)
    print(f"{cond}: grid MSE {mse:.4e}  predicted {pred:.4e}  ratio {mse / pred:.4f}  ({(mse - pred) / se:+.2f} s.e.)  pilots only {pilot_only:.4e}")
    assert abs(mse - pred) <= 4 * se
    assert pred < pilot_only                                                     # 1680 observations beat 24
    assert lmmse_grid_predicted_mse(sim, *cond, m) == pytest.approx(pred, rel=1e-9)


def test_noise_scale_and_the_struct():
    assert data_noise_scale(2) == pytest.approx(1.0, rel=1e-12) and data_noise_scale(4) == pytest.approx(17 / 9, rel=1e-12)
    tb = LmmseTables(CFG)
    g = tb.grid()
    p = g.to_struct(noise_scale=17 / 9)
    want = (17 / 9 * tb.sigma2).astype(np.float32)                               # formed in double, rounded once
    assert [p.noise_var[i] for i in range(p.n_snr)] == [float(v) for v in want]
    assert [tb.to_struct().noise_var[i] for i in range(p.n_snr)] == [float(v) for v in tb.sigma2.astype(np.float32)]
    assert g.gain(2, 1, 3, 2.0) == pytest.approx(1.0 / (g.lam_g[1][:, None] * g.lam_tg[3][None, :] + 2.0 * tb.sigma2[2]))


def test_refusals():
    with pytest.raises(ValueError, match="at most 32"):
        LmmseTables(ChannelSimConfig(ofdm=(12, 33), pilot=(2, 2))).grid()        # T = 33
    LmmseTables(ChannelSimConfig(ofdm=(12, 32), pilot=(2, 2))).grid()            # T = 32 is covered
    tb = LmmseTables(ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3)))
    z = np.zeros((2, 30, 7), dtype=np.complex64)
    with pytest.raises(ValueError, match="shape"):
        lmmse_grid_host(tb, z[:, :29], np.zeros((2, 3)))
    with pytest.raises(ValueError, match="conditions are required"):
        lmmse_grid_host(tb, z, None)
    with pytest.raises(ValueError, match="rows of conditions"):
        lmmse_grid_host(tb, z, np.zeros((3, 3)))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="noise_scale"):
            lmmse_grid_host(tb, z, np.zeros((2, 3)), noise_scale=bad)
    assert np.all(lmmse_grid_host(tb, z, np.zeros((2, 3))) == 0)


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    assert "aft_lmmse_grid_f32" in _abi.SIGNATURES and "aft_lmmse_grid_f32" in _abi.EXPORTED_SYMBOLS
    restype, argtypes = _abi.SIGNATURES["aft_lmmse_grid_f32"]
    assert len(argtypes) == 10 and _abi.AFT_ABI_VERSION == 10
