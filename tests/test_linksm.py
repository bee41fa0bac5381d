"""``linksim``'s spatial-multiplexing link on the CPU: ``link_sm_host`` against NumPy's own linear algebra (the textbook ZF and MMSE
detectors, their post-detection SINR), a brute force over all ``2^m`` symbols, the exact extreme, an unheard second stream against the
diversity link, the weights against the textbook inverse-noise-variance detector, the refusals, the four accumulators and the three
sweeps of ``evaluation`` with ``streams=2`` against the definition applied batch by batch, the binding, the physical orderings, and
the share of flagged decisions on the inputs tests/test_linksm_gpu.py compares the kernel on.

``sm_inputs`` builds those inputs once per grid and ``derived_tau`` / ``derived_e_lambda`` are the bounds the GPU file derives in its
docstring; the GPU file imports both, so both files speak about the same arrays and the same bounds."""
import numpy as np
import pytest
import torch

from adafortitran_amd import _abi
from adafortitran_amd.chansim import SynthLoader, frame_keys, ls_interpolate, simulate_frames_host, words
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DETECTORS, MAX_STREAMS, BlockErrorAccumulator, CodeConfig, HarqAccumulator,
                                      LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator,
                                      branch_weights, constellation, detector_reg, link_decode_host, link_errors_host, link_ldpc_host,
                                      link_llrs_host, link_mrc_host, link_sm_host, llr_scale, noise_sigma, sm_weights)
from adafortitran_amd.lmmse import lmmse_estimate_host
from test_linkmrc import MRC_ODD
from test_linksim import GRIDS, SEED, TAU_CAP

SM_GRIDS = {"default_120x14": 16, "odd_30x7": 32, MRC_ODD: 4}     # frames [0, n) of seed 3
BRANCHES = (2, 3, 4, 8)
SM_SHARE_CAP = 4e-2                                              # of the data (element, axis, stream) triples, at the derived tau(R)
U = 2.0 ** -24
_inputs = {}


def sm_inputs(name):
    """(sim, keys uint64 [n], sigma float32 [n], snr float64 [n], ideal complex64 [n,S,T], {"lmmse": .., "ideal": ..}), made once per
    grid and read-only: ``test_linkmrc.mrc_inputs``' recipe on more frames, each at the SNR it was drawn with."""
    if name not in _inputs:
        sim, n = GRIDS[name][0], SM_GRIDS[name]
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(n))
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        est = {"lmmse": lmmse_estimate_host(sim, pilots, meta).astype(np.complex64), "ideal": ideal}
        keys, sigma, snr = frame_keys(SEED, np.arange(n)), noise_sigma(meta[:, 0]), meta[:, 0].astype(np.float64)
        for a in (ideal, est["lmmse"], keys, sigma, snr):
            a.setflags(write=False)
        _inputs[name] = (sim, keys, sigma, snr, ideal, est)
    return _inputs[name]


def sm_cases():
    """(grid, R, frames used): every R whose groups of 2 R frames fit into the grid's frames, on the frames they fill."""
    return [(name, R, n // (2 * R) * 2 * R) for name, n in SM_GRIDS.items() for R in BRANCHES if n >= 2 * R]


# ---- the bounds of the float32 kernel (derived in the docstring of tests/test_linksm_gpu.py) ----

def _e_m(R: int) -> float:
    """The error of a matched-filter sum in units of its reach, as a complex magnitude."""
    e_x = (1 + U) ** 2 - 1
    e_h = (1 + e_x) * (1 + U) ** 2 - 1
    e_r = (1 + 3 * U) * (1 + 6 * U) * (1 + U) - 1
    e_n = e_r + np.sqrt(2.0) * 8 * U * (1 + e_r)
    e_y = (1 + max(e_h, e_n)) * (1 + U) ** 3 - 1
    e_c = e_y + 2 * U * (1 + e_y)
    return float((1 + e_c) * (1 + U) ** R - 1)


def _e_c_and_e_p(R: int):
    e_m, e_g = _e_m(R), (1 + U) ** (2 + R) - 1              # e_g: g00, g11 and (as a magnitude) g01
    e_a = (1 + e_g) * (1 + U) - 1
    e_t = (1 + e_g) * (1 + e_m) * (1 + 2 * U) - 1
    e_c = (1 + max((1 + e_a) * (1 + e_m) - 1, e_t)) * (1 + U) - 1
    e_n01 = (1 + e_g) ** 2 * (1 + U) ** 2 - 1
    e_p = (1 + max((1 + e_g) * (1 + e_a) - 1, e_n01)) * (1 + U) - 1
    return float(e_c), float(e_p), float(e_a)


def derived_tau(R: int) -> float:
    e_c, e_p, _ = _e_c_and_e_p(R)
    return max(e_c, float((1 + e_p) * (1 + U) ** 3 - 1))


def derived_e_lambda(R: int) -> float:
    e_c, e_p, e_ao = _e_c_and_e_p(R)
    e_a = (1 + U) ** 2 - 1
    e_i = max((1 + e_a) * (1 + e_p), 1 + e_c) * (1 + U) - 1
    e_mu = (1 + e_a) * (1 + U) * (1 + e_i) - 1
    e_d = 2 * e_mu + 2 * U * (1 + e_mu)
    e_eff = (1 + U) / (1 - e_ao) - 1
    return float((1 + e_eff) * (1 + U) * (2 + e_d) - 2)


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    for R in BRANCHES:
        print(f"R = {R}: tau = {derived_tau(R):.3e} = {derived_tau(R) / U:.1f} u, e_lambda = {derived_e_lambda(R):.3e} = "
              f"{derived_e_lambda(R) / U:.1f} u")
    assert derived_tau(2) < derived_tau(3) < derived_tau(8) and derived_e_lambda(2) < derived_e_lambda(8)
    assert derived_tau(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


# ---- the definition rebuilt from the documented streams, with NumPy's own linear algebra ----

def _rebuilt(cfg, keys, ideal, sigma, R):
    """x [G,2,S,T] of the words of frames (0, s) and y [G,R,S,T] of every antenna, from the documented streams: float64."""
    (S, T), m = cfg.sim.ofdm, cfg.bits_per_symbol
    k = keys.reshape(-1, R, 2)
    q = np.arange(S * T, dtype=np.uint64).reshape(1, 1, S, T)
    w = (words(k[:, 0, :, None, None], 5, q) >> np.uint64(64 - m)).astype(np.int64)
    x = constellation(m)[w]
    u1, u2 = (((words(k[:, :, 0, None, None], s, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23 for s in (6, 7))
    noise = sigma.astype(np.float64).reshape(-1, R, 2)[:, :, 0, None, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)
    H = ideal.astype(np.complex128).reshape(-1, R, 2, S, T)
    return x, H[:, :, 0] * x[:, None, 0] + H[:, :, 1] * x[:, None, 1] + noise


def _detected(cfg, y, est, weight, reg, R):
    """The unbiased estimates x^ [G,2,S,T] and the post-detection SINRs [G,2,S,T] of the linear detector with the real weights
    ``weight`` [G,R] and the regulariser ``reg`` [G] (0: zero forcing), by ``np.linalg``: per element ``A = E^H W E + reg I``."""
    S, T = cfg.sim.ofdm
    E = np.moveaxis(est.astype(np.complex128).reshape(-1, R, 2, S, T), (1, 2), (3, 4))      # [G,S,T,R,2]
    yv = np.moveaxis(y, 1, 3)[..., None]                                                     # [G,S,T,R,1]
    W = weight[:, None, None, :, None]
    Eh = np.conj(np.swapaxes(E, -1, -2))
    gram = Eh @ (W * E)
    matched = Eh @ (W * yv)
    eye = np.eye(2)
    xhat, sinr = np.zeros((len(y), 2, S, T), complex), np.zeros((len(y), 2, S, T))
    for g in range(len(y)):
        if reg[g] == 0:                                           # zero forcing: pinv of the weighted channel, SINR 1 / [G^-1]_ss
            sw = np.sqrt(W[g])
            sol = np.linalg.pinv(sw * E[g]) @ (sw * yv[g])
            inv = np.linalg.inv(gram[g])
            xhat[g] = np.moveaxis(sol[..., 0], -1, 0)
            sinr[g] = np.moveaxis(1.0 / np.real(np.diagonal(inv, axis1=-2, axis2=-1)), -1, 0)
        else:                                                     # MMSE, unbiased: (A^-1 m)_s / (A^-1 G)_ss, SINR 1 / (reg [A^-1]_ss) - 1
            inv = np.linalg.inv(gram[g] + reg[g] * eye)
            sol = (inv @ matched[g])[..., 0]
            bias = np.real(np.diagonal(inv @ gram[g], axis1=-2, axis2=-1))
            xhat[g] = np.moveaxis(sol / bias, -1, 0)
            sinr[g] = np.moveaxis(1.0 / (reg[g] * np.real(np.diagonal(inv, axis1=-2, axis2=-1))) - 1.0, -1, 0)
    return xhat, sinr


def _brute_force(cfg, xhat, sinr):
    """[G,2,S,T,m]: min over the symbols with bit 1 minus min over those with bit 0 of ``sinr |x^ - a|^2``."""
    m, pts = cfg.bits_per_symbol, constellation(cfg.bits_per_symbol)
    dist = sinr[..., None] * np.abs(xhat[..., None] - pts) ** 2
    word = np.arange(1 << m)
    out = np.empty((*xhat.shape, m))
    for j in range(m):
        one = ((word >> (m - 1 - j)) & 1).astype(bool)
        out[..., j] = dist[..., one].min(axis=-1) - dist[..., ~one].min(axis=-1)
    return out * cfg.data_mask[None, None, :, :, None]


def _definition_parts(cfg, keys, ideal, est, sigma, rho, scale, reg, R):
    """c_s / p_s and eff_s p_s [G,2,S,T] as the module docstring writes them, on the rebuilt x and y.  ``link_sm_host`` returns neither;
    at m = 2 both are visible in its LLRs (one level pair per axis: Delta = mu_1 - mu_0 = -4 d comp), which is how
    ``test_the_detector_is_the_textbook_one`` ties the two together."""
    S, T = cfg.sim.ofdm
    x, y = _rebuilt(cfg, keys, ideal, sigma, R)
    E = est.astype(np.complex128).reshape(-1, R, 2, S, T)
    w = rho.astype(np.float64).reshape(-1, R, 2)[:, :, 0, None, None]
    g00, g11 = (w * np.abs(E[:, :, 0]) ** 2).sum(1), (w * np.abs(E[:, :, 1]) ** 2).sum(1)
    g01 = (w * E[:, :, 0].conj() * E[:, :, 1]).sum(1)
    m0, m1 = (w * E[:, :, 0].conj() * y).sum(1), (w * E[:, :, 1].conj() * y).sum(1)
    r, s = reg.astype(np.float64)[:, None, None], scale.astype(np.float64)[:, None, None]
    a00, a11 = g00 + r, g11 + r
    c = np.stack([a11 * m0 - g01 * m1, a00 * m1 - g01.conj() * m0], axis=1)
    p = np.stack([g00 * a11 - np.abs(g01) ** 2, g11 * a00 - np.abs(g01) ** 2], axis=1)
    eff = np.stack([s / a11, s / a00], axis=1)
    return c / p, eff * p


def _operands(name, R, which="lmmse", detector="mmse", err_var=0.0):
    sim, keys, sigma, snr, ideal, est = sm_inputs(name)
    n = len(keys) // (2 * R) * 2 * R
    rho, scale, reg = sm_weights(snr[:n], err_var, R, 2, detector)
    return sim, n, keys[:n], sigma[:n], ideal[:n], est[which][:n], rho, scale, reg


@pytest.mark.parametrize("detector", DETECTORS)
def test_the_detector_is_the_textbook_one(detector):
    """``c_s / p_s`` and ``eff_s p_s`` against ``pinv`` / ``inv`` on every data element, to 1e-9 relative; the scales are powers of two so
    that ``reg = 1 / scale`` holds exactly, the weights are the mixed ones of the frames' SNRs."""
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, est, rho, _, _ = _operands(name, R)
        cfg, G = LinkConfig(sim, 4), n // (2 * R)
        scale = (2.0 ** (np.arange(G) % 5 + 1)).astype(np.float32)
        reg = detector_reg(scale, detector)
        assert (reg == 0).all() if detector == "zf" else (reg.astype(np.float64) * scale == 1).all()
        ratio, sinr = _definition_parts(cfg, keys, ideal, est, sigma, rho, scale, reg, R)
        _, y = _rebuilt(cfg, keys, ideal, sigma, R)
        weight = rho.astype(np.float64).reshape(G, R, 2)[:, :, 0]
        xhat, want = _detected(cfg, y, est, weight, reg.astype(np.float64), R)
        if detector == "zf":
            want = want * scale.astype(np.float64)[:, None, None, None]
        mask = cfg.data_mask
        assert (np.abs(ratio - xhat)[..., mask] <= 1e-9 * np.abs(xhat)[..., mask]).all(), (name, R)
        assert (np.abs(sinr - want)[..., mask] <= 1e-9 * want[..., mask]).all() and (want[..., mask] > 0).all(), (name, R)
        # ... and what link_sm_host itself returns is built on exactly these: at m = 2 an axis's LLR is 4 A eff comp
        cfg2 = LinkConfig(sim, 2)
        llr = link_sm_host(cfg2, keys, ideal, est, sigma, rho, scale, reg, R)[2]
        ratio2, sinr2 = _definition_parts(cfg2, keys, ideal, est, sigma, rho, scale, reg, R)
        A = cfg2.d
        want_llr = np.stack([-4 * A * sinr2 * ratio2.real, -4 * A * sinr2 * ratio2.imag], axis=-1) * mask[None, None, :, :, None]
        assert np.abs(llr - want_llr).max() <= 1e-9 * np.abs(want_llr).max()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_llrs_against_a_brute_force_over_all_symbols(m):
    """``eff_s p_s |c_s / p_s - a|^2`` over all 2^m symbols: pins the separable form, the bit order and the scale, to 1e-9 q."""
    for name, R in (("odd_30x7", 2), ("odd_30x7", 3), (MRC_ODD, 2)):
        for detector in DETECTORS:
            sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands(name, R, "lmmse", detector, 0.01)
            cfg = LinkConfig(sim, m)
            out = link_sm_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, e_lambda=TAU_CAP)
            llr, q = out[2], out[5]
            ratio, sinr = _definition_parts(cfg, keys, ideal, est, sigma, rho, scale, reg, R)
            want = _brute_force(cfg, ratio, sinr)
            assert llr.shape == want.shape == q.shape == (n // (2 * R), 2, *sim.ofdm, m)
            assert (np.abs(llr - want) <= 1e-9 * q).all(), (name, R, detector, float((np.abs(llr - want) / np.where(q > 0, q, 1)).max()))
            assert (q[..., cfg.data_mask, :] > 0).all() and (q[..., ~cfg.data_mask, :] == 0).all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_exact_extreme(m):
    """The estimates are the channels, there is no noise and nothing is regularised: no bit error at any m and R."""
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, _, rho, scale, reg = _operands(name, R, "ideal", "zf")
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        counts, loss, llr, wrong, flags = link_sm_host(cfg, keys, ideal, ideal, np.zeros_like(sigma), rho, scale, reg, R, tau=0.0)
        assert counts.shape == (G, 2, 2) and counts.dtype == np.int64 and loss.shape == (G, 2, 1) and llr.shape == (G, 2, *sim.ofdm, m)
        assert not counts.any() and not wrong.any() and wrong.shape == (G, 2, *sim.ofdm) and flags.shape == (G, 2, *sim.ofdm, 2)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_stream_is_the_diversity_link(m):
    """``H_r1 = E_r1 = 0`` and ``reg = 2^-k`` with ``scale = 2^k``: stream 0's counts are ``link_mrc_host``'s on the frames (r, 0) exactly
    and its LLRs to 1e-12 q -- scaling c and p by a power of two changes neither a decision nor a rounding."""
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, est, rho, _, _ = _operands(name, R)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        scale = (2.0 ** (np.arange(G) % 4 + 1)).astype(np.float32)
        reg = (1.0 / scale).astype(np.float32)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        counts, loss, llr, _, _, _, _, _ = link_sm_host(cfg, keys, H, E, sigma, rho, scale, reg, R, 2, (1.0, 0.5), tau=TAU_CAP, e_lambda=TAU_CAP)
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R, (1.0, 0.5), e_lambda=TAU_CAP)
        assert np.array_equal(counts[:, 0], want[0]), (name, R)
        assert (np.abs(llr[:, 0] - want[2]) <= 1e-12 * want[5]).all(), (name, R)
        np.testing.assert_allclose(loss[:, 0], want[1], rtol=1e-9, atol=0)
        # the unheard stream: c_1 = p_1 = 0, so every LLR is 0 and every bit costs one bit
        assert not llr[:, 1].any() and np.allclose(loss[:, 1], m * cfg.data_elements)


@pytest.mark.parametrize("m", (2, 6))
@pytest.mark.parametrize("detector", DETECTORS)
def test_mixed_snr_is_the_detector_with_inverse_noise_variances(detector, m):
    """The textbook detector in float64 with ``W = diag(1 / sigma_r^2)``, ``sigma_r^2 = 10^(-snr_r / 10)``, and ``reg = 1`` in those units
    (MMSE for unit-energy symbols).  The definition differs from it by the float32 roundings of ``rho``, ``scale``, ``reg`` and (in the
    noise) ``sigma``: each within 2^-24, a few 1e-7 of a metric in all -- hence 1e-6 of ``q``."""
    R = 4
    sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands("odd_30x7", R, "lmmse", detector)
    snr = sm_inputs("odd_30x7")[3][:n]
    cfg, G = LinkConfig(sim, m), n // (2 * R)
    assert rho.reshape(G, R, 2)[:, :, 0].max() > 10 and rho.reshape(G, R, 2)[:, :, 0].min() < 0.5      # the SNRs are mixed
    out = link_sm_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, e_lambda=TAU_CAP)
    _, y = _rebuilt(cfg, keys, ideal, sigma, R)
    weight = (10.0 ** (snr / 10.0)).reshape(G, R, 2)[:, :, 0]
    xhat, sinr = _detected(cfg, y, est, weight, np.zeros(G) if detector == "zf" else np.ones(G), R)
    want = _brute_force(cfg, xhat, sinr)
    assert (np.abs(out[2] - want) <= 1e-6 * out[5]).all()


def test_the_weights_and_the_regulariser():
    snr = np.array([0.0, 25.0, 10.0, 10.0, 30.0, 5.0, 7.0, 7.0])
    for err_var in (0.0, 0.02):
        rho, scale, reg = sm_weights(snr, err_var, 2, 2, "mmse")
        assert rho.dtype == scale.dtype == reg.dtype == np.float32 and rho.shape == (8,) and scale.shape == reg.shape == (2,)
        s = llr_scale(snr, err_var)
        assert scale.tobytes() == s[::4].tobytes() and rho.tobytes() == branch_weights(snr, err_var, 4)[0].tobytes()
        assert reg.tobytes() == (1.0 / s[::4].astype(np.float64)).astype(np.float32).tobytes()
        assert not sm_weights(snr, err_var, 2, 2, "zf")[2].any()
    assert sm_weights(snr, 0.0, 4)[1].shape == (1,)


def test_refusals():
    sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands("odd_30x7", 4)
    cfg = LinkConfig(sim, 4)
    for bad in (1, 3, 0, 2.0, True, "2"):
        with pytest.raises(ValueError, match="streams"):
            link_sm_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, 4, bad)
        with pytest.raises(ValueError, match="streams"):
            sm_weights(np.zeros(8), 0.0, 2, bad)
    for bad in (0, 3, 2.0, True, "2"):
        with pytest.raises(ValueError, match="streams"):
            LinkAccumulator(cfg, "cpu", branches=2, streams=bad)
    for bad in (0, 9, 2.0, -1, True, "2"):
        with pytest.raises(ValueError, match="branches"):
            link_sm_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, bad)
    with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
        link_sm_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, 1)
    for make in (lambda: LinkAccumulator(cfg, "cpu", streams=2), lambda: RateAccumulator(cfg, "cpu", branches=1, streams=2),
                 lambda: BlockErrorAccumulator(CodeConfig(cfg, 64), "cpu", streams=2)):
        with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
            make()
    assert MAX_STREAMS == 2
    with pytest.raises(ValueError, match="32 frames is not a multiple of branches \\* streams = 3 \\* 2"):
        link_sm_host(cfg, keys, ideal, ideal, sigma, rho, scale, reg, 3)
    with pytest.raises(ValueError, match="rho"):
        link_sm_host(cfg, keys, ideal, ideal, sigma, rho[:8], scale, reg, 4)
    with pytest.raises(ValueError, match="scale"):
        link_sm_host(cfg, keys, ideal, ideal, sigma, rho, scale[:3], reg, 4)
    with pytest.raises(ValueError, match="reg"):
        link_sm_host(cfg, keys, ideal, ideal, sigma, rho, scale, np.repeat(reg, 2), 4)
    for bad in ("ml", "ZF", None, 0):
        with pytest.raises(ValueError, match="detector"):
            detector_reg(scale, bad)
        with pytest.raises(ValueError, match="detector"):
            LinkAccumulator(cfg, "cpu", branches=2, streams=2, detector=bad)
    LinkAccumulator(cfg, "cpu", detector="anything")                            # one stream ignores the detector
    for make in (lambda: LinkAccumulator(cfg, "cpu", branches=2, streams=2), lambda: RateAccumulator(cfg, "cpu", branches=2, streams=2),
                 lambda: BlockErrorAccumulator(CodeConfig(cfg, 64), "cpu", branches=2, streams=2)):
        with pytest.raises(ValueError, match="6 frames is not a multiple of branches \\* streams = 2 \\* 2"):
            make().update(None, torch.from_numpy(ideal[:6].copy()), frame_ids=np.arange(6), snr_db=np.zeros(6))
    # the HARQ accumulator has no streams: its rounds are consecutive LLR frames, which would be the two streams of one group
    import inspect
    assert "streams" not in inspect.signature(HarqAccumulator.__init__).parameters
    assert "streams" in inspect.signature(LdpcBlockErrorAccumulator.__init__).parameters


class _Ls(torch.nn.Module):
    """The LS-interpolated estimate as a model ``evaluation.forward_pass`` can call."""

    def __init__(self, sim):
        super().__init__()
        self.sim = sim
        self.register_buffer("anchor", torch.zeros(1))

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.numpy()))


@pytest.mark.parametrize("detector", DETECTORS)
def test_accumulators_and_sweeps_with_two_streams_on_the_host(detector):
    """A host ``SynthLoader`` (every frame at its own SNR), three batches of eight frames (two groups of 2 x 2): each accumulator and
    each sweep equals the definition applied batch by batch, the coded ones through the host decoders on the definition's LLRs rounded
    to float32 with the keys of frames (0, s)."""
    from adafortitran_amd.evaluation import get_link_bler, get_link_rates, get_link_stats
    R, N, seed, err_var = 2, 2, 5, 0.01
    sim = GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code, ldpc = CodeConfig(cfg, 64, "1/2"), LdpcConfig(cfg, (3, 6))
    factors = (1.0, 0.5)
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 8, 24, device="cpu", seed=seed))
    assert len(batches) == 3
    kw = dict(branches=R, streams=N, detector=detector)
    hard, rate = LinkAccumulator(cfg, "cpu", seed, **kw), RateAccumulator(cfg, "cpu", seed, factors, err_var, **kw)
    conv, lay = BlockErrorAccumulator(code, "cpu", seed, err_var, **kw), LdpcBlockErrorAccumulator(ldpc, "cpu", seed, err_var, R, N, detector)
    want = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "loss0": np.zeros(8), "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64),
            "conv0": np.zeros(2, np.int64)}
    for pilots, ideal, meta in batches:
        est = model(pilots)
        for acc in (hard, rate, conv, lay):
            acc.update(est, ideal, meta)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        sent_keys = np.ascontiguousarray(keys.reshape(-1, R, N)[:, 0, :]).reshape(-1)
        snr = meta[1].numpy().reshape(-1)
        for ev, tag in ((0.0, "0"), (err_var, "")):
            rho, scale, reg = sm_weights(snr, ev, R, N, detector)
            counts, loss, llr = (v.reshape(-1, *v.shape[2:]) for v in link_sm_host(
                cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), rho, scale, reg, R, N,
                factors if tag == "" else np.asarray([2.0 ** -k for k in range(8)])))
            if tag == "0":
                want["hard"] += counts.sum(axis=0)
                want["loss0"] += loss.sum(axis=0)
                want["conv0"] += link_decode_host(code, sent_keys, llr.astype(np.float32))[0].sum(axis=0)
            else:
                want["loss"] += loss.sum(axis=0)
                want["conv"] += link_decode_host(code, sent_keys, llr.astype(np.float32))[0].sum(axis=0)
                want["ldpc"] += link_ldpc_host(ldpc, sent_keys, llr.astype(np.float32))[0].sum(axis=0)
    F = 12                                                                       # frames counts G N: per stream
    assert hard.frames == rate.frames == conv.frames == lay.frames == F
    assert hard.errors.tolist() == want["hard"].tolist() and hard.result() == want["hard"][0] / (F * cfg.bits_per_frame)
    assert hard.result_ser() == want["hard"][1] / (F * cfg.data_elements)
    assert np.array_equal(rate.loss.numpy(), want["loss"])
    assert rate.result() == [4 - v / (F * cfg.data_elements) for v in want["loss"]]
    assert conv.errors.tolist() == want["conv"].tolist() and conv.result() == want["conv"][1] / (F * code.blocks)
    assert lay.errors.tolist() == want["ldpc"].tolist() and lay.result() == want["ldpc"][1] / (F * ldpc.blocks)
    assert lay.result_throughput() == (F * ldpc.blocks - want["ldpc"][1]) * ldpc.info_bits / (F * cfg.data_elements)
    assert 0 < want["hard"][0] < F * cfg.bits_per_frame // 2                       # the frames are not trivial
    # the sweeps (err_var 0 unless given), over a loader that replays the same frames
    loaders = [("SNR_0", SynthLoader(sim, 8, 24, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_stats(model, loaders, cfg, seed, **kw) == {0: want["hard"][0] / (F * cfg.bits_per_frame)}
    assert get_link_rates(model, loaders, cfg, seed, **kw) == {0: max(4 - v / (F * cfg.data_elements) for v in want["loss0"])}
    assert get_link_bler(model, loaders, code, seed, **kw) == {0: want["conv0"][1] / (F * code.blocks)}
    assert get_link_bler(model, loaders, ldpc, seed, err_var, **kw) == {0: want["ldpc"][1] / (F * ldpc.blocks)}


def test_one_stream_objects_are_todays():
    """``streams=1`` (and any detector) is the path the accumulators had: the same numbers as the objects made without the arguments."""
    from adafortitran_amd.evaluation import get_link_stats
    seed, sim = 5, GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code = CodeConfig(cfg, 64, "1/2")
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 4, 8, device="cpu", seed=seed))
    for R in (1, 2):
        pairs = [(LinkAccumulator(cfg, "cpu", seed, R), LinkAccumulator(cfg, "cpu", seed, R, 1, "zf")),
                 (RateAccumulator(cfg, "cpu", seed, (1.0, 0.5), 0.01, R), RateAccumulator(cfg, "cpu", seed, (1.0, 0.5), 0.01, R, 1, "zf")),
                 (BlockErrorAccumulator(code, "cpu", seed, 0.01, R), BlockErrorAccumulator(code, "cpu", seed, 0.01, R, streams=1))]
        for pilots, ideal, meta in batches:
            for a, b in pairs:
                a.update(model(pilots), ideal, meta)
                b.update(model(pilots), ideal, meta)
        for a, b in pairs:
            assert a.frames == b.frames == 8 // R and b.streams == 1 and a.result() == b.result()
        assert pairs[0][0].errors.tolist() == pairs[0][1].errors.tolist() and torch.equal(pairs[1][0].loss, pairs[1][1].loss)
    loaders = [("SNR_0", SynthLoader(sim, 4, 8, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_stats(model, loaders, cfg, seed, branches=2) == get_link_stats(model, loaders, cfg, seed, branches=2, streams=1)
    # and the host definitions the single-stream accumulators call have not moved
    keys = frame_keys(seed, np.arange(4))
    pilots, ideal, meta = batches[0]
    snr = meta[1].numpy().reshape(-1)
    got = LinkAccumulator(cfg, "cpu", seed)
    got.update(model(pilots), ideal, meta)
    ids = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
    assert got.errors.tolist() == link_errors_host(cfg, frame_keys(seed, ids), ideal.numpy(), model(pilots).numpy(), noise_sigma(snr)).sum(0).tolist()
    assert len(keys) == 4 and link_llrs_host(cfg, keys, ideal.numpy(), ideal.numpy(), noise_sigma(snr), llr_scale(snr))[1].shape == (4, 30, 7, 4)


def test_the_entry_point_is_in_the_signature_table_and_the_abi_version_stays():
    import ctypes as C
    assert _abi.AFT_ABI_VERSION == 10 and _abi.AFT_LINK_MAX_STREAMS == 2 and _abi.AFT_LINK_MAX_BRANCHES == 8
    restype, argtypes = _abi.SIGNATURES["aft_link_sm_f32"]
    assert "aft_link_sm_f32" in _abi.EXPORTED_SYMBOLS and restype is C.c_int and len(argtypes) == 17
    assert argtypes[0]._type_ is _abi.AftLink and [i for i, t in enumerate(argtypes) if t is C.c_int] == [9, 10, 11, 15]
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_sm_f32") == names.index("aft_link_harq_f32") + 1                  # the header's order


def test_physical_orderings():
    """Asserted is the ordering only; the values are printed.  One simulated pack of 64 frames at 15 dB, 16-QAM (the pack of the GPU
    file's sweep): 16, 8 and 4 groups at R = 2, 4 and 8."""
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    pack = make_pack(sim, 64, seed=31, snr_db=15.0)
    ideal, snr = pack["h_ideal"], pack["meta"][:, 1].astype(np.float64)
    pilots = pack["h_ls_sparse"][:, np.asarray(sim.pilot_scs)][:, :, np.asarray(sim.pilot_symbols)]
    est = {"perfect": ideal, "lmmse": lmmse_estimate_host(sim, pilots, pack["meta"][:, 1:4]).astype(np.complex64), "ls": pack["h_ls_full"]}
    keys, sigma = frame_keys(1, np.arange(64)), noise_sigma(snr)
    ber, streams = {}, {}
    for R in (2, 4, 8):
        for d in DETECTORS:
            rho, scale, reg = sm_weights(snr, 0.0, R, 2, d)
            for w, e in est.items():
                counts = link_sm_host(cfg, keys, ideal, e, sigma, rho, scale, reg, R)[0]
                ber[R, d, w] = float(counts[..., 0].sum()) / (counts.shape[0] * 2 * cfg.bits_per_frame)
                streams[R, d, w] = counts[..., 0].sum(axis=0)
    print({k: round(v, 5) for k, v in ber.items()})
    for d in DETECTORS:
        for w in est:
            assert ber[2, d, w] > ber[4, d, w] > ber[8, d, w]                           # BER falls with R
        for R in (2, 4, 8):
            assert ber[R, d, "perfect"] <= ber[R, d, "lmmse"] <= ber[R, d, "ls"]
    for w in est:
        assert ber[2, "mmse", w] <= ber[2, "zf", w]
    # each stream against the 1 x R diversity link on the same antennas: the frames (r, s) of each group, stream s alone on the air
    for R in (2, 4, 8):
        for s in (0, 1):
            pick = np.arange(64).reshape(-1, R, 2)[:, :, s].reshape(-1)
            w, c = branch_weights(snr[pick], 0.0, R)
            alone = link_mrc_host(cfg, keys[pick], ideal[pick], est["lmmse"][pick], sigma[pick], w, c, R)[0][:, 0].sum()
            print(f"R = {R}, stream {s}: bit errors {int(streams[R, 'mmse', 'lmmse'][s])} at 2 x {R}, {int(alone)} at 1 x {R}")
            assert streams[R, "mmse", "lmmse"][s] >= alone and streams[R, "zf", "lmmse"][s] >= alone


def sm_flagged_share(cfg, flags):
    triples = 2 * cfg.data_elements * flags.shape[0] * flags.shape[1]
    return float(flags.sum()) / triples if triples else 0.0


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_flagged_share_on_the_inputs_the_gpu_tests_use(m):
    """At most 4e-2 of the data (element, axis, stream) triples at the derived tau(R), for every grid, R, detector and estimate.  The
    cancellation in ``p_s`` makes it larger than the one-stream links' 1e-3 (module docstring of ``linksim``)."""
    worst = (0.0, None)
    for name, R, _ in sm_cases():
        for detector in DETECTORS:
            for which in ("lmmse", "ideal"):
                sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands(name, R, which, detector)
                cfg = LinkConfig(sim, m)
                flags = link_sm_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, tau=derived_tau(R))[4]
                share = sm_flagged_share(cfg, flags)
                assert share <= SM_SHARE_CAP, (name, R, detector, which, share)
                worst = max(worst, (share, (name, R, detector, which)))
    print(f"m = {m}: the largest flagged share at tau(R) is {worst[0]:.2e} at {worst[1]}")
