"""``linksim``'s joint link on the CPU: ``link_joint_host`` against a brute force over all ``M^2`` symbol pairs (in the Gram form and as
the literal weighted residual rebuilt from the documented streams), the hard counts as the sign rule on the LLRs, an unheard second
stream against the diversity link, the refusals, the four accumulators and the three sweeps of ``evaluation`` with
``detector="joint"`` against the definition applied batch by batch, the binding, and the share of flagged bits and elements on the
inputs tests/test_linkjoint_gpu.py compares the kernel on.

``derived_tau_joint`` / ``derived_e_lambda_joint`` are the bounds the GPU file derives in its docstring; the GPU file imports them, so
both files speak about the same arrays (``test_linksm.sm_inputs``) and the same bounds."""
import numpy as np
import pytest
import torch

from adafortitran_amd import _abi
from adafortitran_amd.chansim import SynthLoader, frame_keys, words
from adafortitran_amd.linksim import (ALL_DETECTORS, BITS_PER_SYMBOL, DETECTORS, JOINT_DETECTOR, BlockErrorAccumulator, CodeConfig,
                                      HarqAccumulator, LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig,
                                      RateAccumulator, constellation, detector_reg, link_decode_host, link_joint_host, link_ldpc_host,
                                      link_mrc_host, noise_sigma, sm_weights)
from test_linkmrc import MRC_ODD
from test_linksim import GRIDS, TAU_CAP
from test_linksm import SM_SHARE_CAP, U, _e_m, _Ls, _rebuilt, sm_cases, sm_inputs

JOINT_ELEMENT_SHARE_CAP = 1.5e-1                                 # of the data (element, stream) pairs with any flagged bit


# ---- the bounds of the float32 kernel (derived in the docstring of tests/test_linkjoint_gpu.py) ----

def _e_f(R: int) -> float:
    """The error of a candidate's metric f in units of Q."""
    e_m, e_g, e_a = _e_m(R), (1 + U) ** (2 + R) - 1, (1 + U) ** 2 - 1
    e_p = (1 + e_a) ** 2 * (1 + e_g) * (1 + U) ** 2 - 1         # a_k^2 g: two levels, the sum, two roundings
    e_t = max(e_p, (1 + e_a) * (1 + e_m) * (1 + U) ** 2 - 1)
    e_z = (1 + max(e_m, (1 + e_g) * (1 + e_a) - 1)) * (1 + U) ** 2 - 1
    e_r = max((1 + e_p) * (1 + U) - 1, (1 + e_a) * (1 + U) * (1 + e_z) - 1)
    return float((1 + max(e_t, e_r)) * (1 + U) ** 2 - 1)


def derived_tau_joint(R: int) -> float:
    e_f = _e_f(R)
    return float(2 * e_f + 2 * U * (1 + e_f))


def derived_e_lambda_joint(R: int) -> float:
    tau = derived_tau_joint(R)
    return float(tau + U * (2 + tau))


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    for R in (2, 3, 4, 8):
        print(f"R = {R}: tau = {derived_tau_joint(R):.3e} = {derived_tau_joint(R) / U:.1f} u, e_lambda = {derived_e_lambda_joint(R):.3e} = "
              f"{derived_e_lambda_joint(R) / U:.1f} u")
    assert derived_tau_joint(2) < derived_tau_joint(3) < derived_tau_joint(8) and derived_e_lambda_joint(2) < derived_e_lambda_joint(8)
    assert derived_tau_joint(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda_joint(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP
    assert derived_tau_joint(2) > 40 * U                          # two metrics of some twenty roundings each: not vacuous


# ---- the brute force over all pairs, on the streams rebuilt from their documentation ----

def _operands(name, R, which="lmmse", err_var=0.0, groups=None):
    sim, keys, sigma, snr, ideal, est = sm_inputs(name)
    n = len(keys) // (2 * R) * 2 * R if groups is None else groups * 2 * R
    rho, scale, _ = sm_weights(snr[:n], err_var, R, 2, "zf")
    return sim, n, keys[:n], sigma[:n], ideal[:n], est[which][:n], rho, scale


def _pair_metrics(cfg, keys, ideal, est, sigma, rho, R, form):
    """[G,S,T,M,M]: the metric of every pair (word of stream 0, word of stream 1).  ``"gram"``: ``g00 |x_0|^2 + g11 |x_1|^2 -
    2 Re(conj(x_0) m_0) - 2 Re(conj(x_1) m_1) + 2 Re(conj(x_0) g01 x_1)``; ``"residual"``: the literal ``sum_r rho_r |y_r - E_r0 x_0 -
    E_r1 x_1|^2``.  They differ by ``sum_r rho_r |y_r|^2``, which no difference of minima sees."""
    S, T = cfg.sim.ofdm
    pts = constellation(cfg.bits_per_symbol)
    _, y = _rebuilt(cfg, keys, ideal, sigma, R)                                   # [G,R,S,T]
    E = est.astype(np.complex128).reshape(-1, R, 2, S, T)
    w = rho.astype(np.float64).reshape(-1, R, 2)[:, :, 0, None, None]
    x0, x1 = pts[:, None], pts[None, :]
    if form == "residual":
        out = 0.0
        for r in range(R):
            res = y[:, r, ..., None, None] - E[:, r, 0, ..., None, None] * x0 - E[:, r, 1, ..., None, None] * x1
            out = out + w[:, r, ..., None, None] * (res.real ** 2 + res.imag ** 2)
        return out
    g00, g11 = (w * np.abs(E[:, :, 0]) ** 2).sum(1), (w * np.abs(E[:, :, 1]) ** 2).sum(1)
    g01 = (w * E[:, :, 0].conj() * E[:, :, 1]).sum(1)
    m0, m1 = (w * E[:, :, 0].conj() * y).sum(1), (w * E[:, :, 1].conj() * y).sum(1)
    wide = lambda v: v[..., None, None]  # noqa: E731
    return (wide(g00) * np.abs(x0) ** 2 + wide(g11) * np.abs(x1) ** 2 - 2 * (np.conj(x0) * wide(m0)).real - 2 * (np.conj(x1) * wide(m1)).real
            + 2 * (np.conj(x0) * wide(g01) * x1).real)


def _brute_force(cfg, metric):
    """[G,2,S,T,m]: per stream and bit of its word, the minimum over the pairs with the bit 1 minus the minimum over those with it 0."""
    m = cfg.bits_per_symbol
    word = np.arange(1 << m)
    best = (metric.min(axis=-1), metric.min(axis=-2))                            # per word of stream 0; per word of stream 1
    out = np.empty((metric.shape[0], 2, *metric.shape[1:3], m))
    for e in (0, 1):
        for j in range(m):
            one = ((word >> (m - 1 - j)) & 1).astype(bool)
            out[:, e, ..., j] = best[e][..., one].min(axis=-1) - best[e][..., ~one].min(axis=-1)
    return out * cfg.data_mask[None, None, :, :, None]


BRUTE_CASES = [(2, "odd_30x7", 2, None), (2, "odd_30x7", 3, None), (4, "odd_30x7", 2, None), (4, "odd_30x7", 3, None),
               (6, "odd_30x7", 2, 1), (8, MRC_ODD, 2, None)]


@pytest.mark.parametrize("form", ("gram", "residual"))
@pytest.mark.parametrize("m,name,R,groups", BRUTE_CASES)
def test_delta_against_a_brute_force_over_all_pairs(m, name, R, groups, form):
    """``2 M`` candidates with a separable inner minimum against all ``M^2`` pairs: pins the metric, ``g_oe``, the bit order and the
    scale, to 1e-10 of ``q = scale Q``."""
    sim, n, keys, sigma, ideal, est, rho, scale = _operands(name, R, "lmmse", 0.01, groups)
    cfg = LinkConfig(sim, m)
    out = link_joint_host(cfg, keys, ideal, est, sigma, rho, scale, R, e_lambda=TAU_CAP)
    llr, q = out[2], out[5]
    want = _brute_force(cfg, _pair_metrics(cfg, keys, ideal, est, sigma, rho, R, form))
    want = want * scale.astype(np.float64)[:, None, None, None, None]
    assert llr.shape == want.shape == q.shape == (n // (2 * R), 2, *sim.ofdm, m)
    worst = float((np.abs(llr - want) / np.where(q > 0, q, 1)).max())
    print(f"m = {m}, {name}, R = {R}, {form}: largest |Lambda - brute force| / q = {worst:.2e}")
    assert (np.abs(llr - want) <= 1e-10 * q).all(), worst
    assert (q[..., cfg.data_mask, :] > 0).all() and (q[..., ~cfg.data_mask, :] == 0).all()
    assert np.abs(llr[..., cfg.data_mask, :]).max() > 0 and not llr[..., ~cfg.data_mask, :].any()
    assert (np.abs(llr) <= 2 * q).all()                                           # |f| <= Q, so |Delta| <= 2 Q


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_hard_counts_are_the_sign_rule_on_the_llrs(m):
    total = 0
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, est, rho, scale = _operands(name, R)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        (S, T) = sim.ofdm
        counts, loss, llr, wrong, flags = link_joint_host(cfg, keys, ideal, est, sigma, rho, scale, R, tau=0.0)
        assert counts.shape == (G, 2, 2) and counts.dtype == np.int64 and loss.shape == (G, 2, 1) and llr.shape == (G, 2, S, T, m)
        assert wrong.shape == (G, 2, S, T) and flags.shape == (G, 2, S, T, m) and flags.dtype == bool
        q = np.arange(S * T, dtype=np.uint64).reshape(1, 1, S, T)
        w = (words(keys.reshape(G, R, 2)[:, 0, :, None, None], 5, q) >> np.uint64(64 - m)).astype(np.int64)     # the sent words
        sent = np.stack([(w >> (m - 1 - j)) & 1 for j in range(m)], axis=-1)
        differ = ((llr < 0).astype(np.int64) != sent) & cfg.data_mask[None, None, :, :, None]
        assert np.array_equal(wrong, differ.sum(axis=-1))
        assert np.array_equal(counts[..., 0], wrong.sum(axis=(2, 3))) and np.array_equal(counts[..., 1], (wrong > 0).sum(axis=(2, 3)))
        total += int(counts[..., 0].sum())
        assert counts[..., 0].sum() < G * cfg.bits_per_frame
        # the loss is the soft link's on these LLRs
        z = np.where(sent == 1, llr, -llr)
        np.testing.assert_allclose(loss[..., 0], (np.logaddexp(0.0, z) * cfg.data_mask[None, None, :, :, None]).sum(axis=(2, 3, 4))
                                   / np.log(2.0), rtol=1e-12)
    assert total > 0                                                              # the frames are not trivial


def test_the_exact_extreme_and_all_zero_estimates():
    """The estimates are the channels and there is no noise: no bit error at any m and R.  All-zero estimates: every LLR is 0."""
    for m in BITS_PER_SYMBOL:
        for name, R, n in sm_cases():
            sim, n, keys, sigma, ideal, _, rho, scale = _operands(name, R, "ideal")
            cfg = LinkConfig(sim, m)
            counts, _, llr = link_joint_host(cfg, keys, ideal, ideal, np.zeros_like(sigma), rho, scale, R)
            assert not counts.any() and np.isfinite(llr).all()
            if name == "default_120x14":
                continue
            _, loss, llr = link_joint_host(cfg, keys, ideal, np.zeros_like(ideal), sigma, rho, scale, R)
            assert not llr.any() and np.allclose(loss, m * cfg.data_elements)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_stream(m):
    """``H_r1 = E_r1 = 0``: stream 1's Delta is exactly 0, and stream 0's LLRs are ``link_mrc_host``'s on the frames (r, 0) to 1e-12 of
    ``q`` (the joint link's ``q``, which is the larger: it carries sqrt(2) where the diversity link's reach carries 1)."""
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, est, rho, scale = _operands(name, R)
        cfg = LinkConfig(sim, m)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        counts, loss, llr, _, _, _, _, q = link_joint_host(cfg, keys, H, E, sigma, rho, scale, R, 2, (1.0, 0.5), tau=TAU_CAP, e_lambda=TAU_CAP)
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R, (1.0, 0.5), e_lambda=TAU_CAP)
        assert (llr[:, 1] == 0).all() and np.allclose(loss[:, 1], m * cfg.data_elements)
        assert (np.abs(llr[:, 0] - want[2]) <= 1e-12 * q[:, 0]).all(), (name, R)
        assert np.abs(want[2]).max() > 0 and (q[:, 0] >= want[5]).all()
        np.testing.assert_allclose(loss[:, 0], want[1], rtol=1e-9, atol=0)


def test_refusals_and_names():
    sim, n, keys, sigma, ideal, est, rho, scale = _operands("odd_30x7", 4)
    cfg = LinkConfig(sim, 4)
    assert JOINT_DETECTOR == "joint" and DETECTORS == ("zf", "mmse") and ALL_DETECTORS == ("zf", "mmse", "joint")
    for bad in (1, 3, 0, 2.0, True, "2"):
        with pytest.raises(ValueError, match="streams"):
            link_joint_host(cfg, keys, ideal, ideal, sigma, rho, scale, 4, bad)
    for bad in (0, 9, 2.0, -1, True, "2"):
        with pytest.raises(ValueError, match="branches"):
            link_joint_host(cfg, keys, ideal, ideal, sigma, rho, scale, bad)
    with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
        link_joint_host(cfg, keys, ideal, ideal, sigma, rho, scale, 1)
    with pytest.raises(ValueError, match="32 frames is not a multiple of branches \\* streams = 3 \\* 2"):
        link_joint_host(cfg, keys, ideal, ideal, sigma, rho, scale, 3)
    with pytest.raises(ValueError, match="rho"):
        link_joint_host(cfg, keys, ideal, ideal, sigma, rho[:8], scale, 4)
    with pytest.raises(ValueError, match="scale"):
        link_joint_host(cfg, keys, ideal, ideal, sigma, rho, scale[:3], 4)
    with pytest.raises(ValueError, match="between 1 and 8 factors"):
        link_joint_host(cfg, keys, ideal, ideal, sigma, rho, scale, 4, 2, np.ones(9))
    # the regulariser stays the linear detectors': "joint" has none, and "ml" stays refused everywhere
    for bad in ("joint", "ml"):
        with pytest.raises(ValueError, match="detector"):
            detector_reg(scale, bad)
        with pytest.raises(ValueError, match="detector"):
            sm_weights(np.zeros(8), 0.0, 2, 2, bad)
    for bad in ("ml", "JOINT", "sphere", None):
        with pytest.raises(ValueError, match="detector"):
            LinkAccumulator(cfg, "cpu", branches=2, streams=2, detector=bad)
    for make in (lambda: LinkAccumulator(cfg, "cpu", streams=2, detector="joint"),
                 lambda: RateAccumulator(cfg, "cpu", branches=1, streams=2, detector="joint"),
                 lambda: BlockErrorAccumulator(CodeConfig(cfg, 64), "cpu", streams=2, detector="joint")):
        with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
            make()
    for make in (lambda: LinkAccumulator(cfg, "cpu", branches=2, streams=2, detector="joint"),
                 lambda: RateAccumulator(cfg, "cpu", branches=2, streams=2, detector="joint"),
                 lambda: BlockErrorAccumulator(CodeConfig(cfg, 64), "cpu", branches=2, streams=2, detector="joint")):
        with pytest.raises(ValueError, match="6 frames is not a multiple of branches \\* streams = 2 \\* 2"):
            make().update(None, torch.from_numpy(ideal[:6].copy()), frame_ids=np.arange(6), snr_db=np.zeros(6))
    LinkAccumulator(cfg, "cpu", detector="joint")                                # one stream ignores the detector
    import inspect
    assert "streams" not in inspect.signature(HarqAccumulator.__init__).parameters


def test_accumulators_and_sweeps_with_the_joint_detector_on_the_host():
    """``test_linksm``'s host sweep with ``detector="joint"``: each accumulator and each sweep equals ``link_joint_host`` applied batch by
    batch, the coded ones through the host decoders on its LLRs rounded to float32 with the keys of frames (0, s)."""
    from adafortitran_amd.evaluation import get_link_bler, get_link_rates, get_link_stats
    R, N, seed, err_var = 2, 2, 5, 0.01
    sim = GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 4)
    code, ldpc = CodeConfig(cfg, 64, "1/2"), LdpcConfig(cfg, (3, 6))
    factors = (1.0, 0.5)
    model = _Ls(sim)
    batches = list(SynthLoader(sim, 8, 24, device="cpu", seed=seed))
    kw = dict(branches=R, streams=N, detector="joint")
    hard, rate = LinkAccumulator(cfg, "cpu", seed, **kw), RateAccumulator(cfg, "cpu", seed, factors, err_var, **kw)
    conv, lay = BlockErrorAccumulator(code, "cpu", seed, err_var, **kw), LdpcBlockErrorAccumulator(ldpc, "cpu", seed, err_var, R, N, "joint")
    mmse = LinkAccumulator(cfg, "cpu", seed, branches=R, streams=N)
    want = {"hard": np.zeros(2, np.int64), "loss": np.zeros(2), "loss0": np.zeros(8), "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64),
            "conv0": np.zeros(2, np.int64)}
    for pilots, ideal, meta in batches:
        est = model(pilots)
        for acc in (hard, rate, conv, lay, mmse):
            acc.update(est, ideal, meta)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        sent_keys = np.ascontiguousarray(keys.reshape(-1, R, N)[:, 0, :]).reshape(-1)
        snr = meta[1].numpy().reshape(-1)
        for ev, tag in ((0.0, "0"), (err_var, "")):
            rho, scale, _ = sm_weights(snr, ev, R, N)
            counts, loss, llr = (v.reshape(-1, *v.shape[2:]) for v in link_joint_host(
                cfg, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), rho, scale, R, N,
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
    assert hard.frames == rate.frames == conv.frames == lay.frames == F and hard.detector == "joint"
    assert hard.errors.tolist() == want["hard"].tolist() and hard.result() == want["hard"][0] / (F * cfg.bits_per_frame)
    assert hard.result_ser() == want["hard"][1] / (F * cfg.data_elements)
    assert np.array_equal(rate.loss.numpy(), want["loss"])
    assert rate.result() == [4 - v / (F * cfg.data_elements) for v in want["loss"]]
    assert conv.errors.tolist() == want["conv"].tolist() and conv.result() == want["conv"][1] / (F * code.blocks)
    assert lay.errors.tolist() == want["ldpc"].tolist() and lay.result() == want["ldpc"][1] / (F * ldpc.blocks)
    assert 0 < want["hard"][0] < F * cfg.bits_per_frame // 2 and hard.errors.tolist() != mmse.errors.tolist()
    loaders = [("SNR_0", SynthLoader(sim, 8, 24, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_stats(model, loaders, cfg, seed, **kw) == {0: want["hard"][0] / (F * cfg.bits_per_frame)}
    assert get_link_rates(model, loaders, cfg, seed, **kw) == {0: max(4 - v / (F * cfg.data_elements) for v in want["loss0"])}
    assert get_link_bler(model, loaders, code, seed, **kw) == {0: want["conv0"][1] / (F * code.blocks)}
    assert get_link_bler(model, loaders, ldpc, seed, err_var, **kw) == {0: want["ldpc"][1] / (F * ldpc.blocks)}


def test_the_entry_point_is_in_the_signature_table_next_after_the_linear_detector():
    import ctypes as C
    import os
    import re
    assert _abi.AFT_ABI_VERSION == 10
    restype, argtypes = _abi.SIGNATURES["aft_link_joint_f32"]
    sm = _abi.SIGNATURES["aft_link_sm_f32"][1]
    assert "aft_link_joint_f32" in _abi.EXPORTED_SYMBOLS and restype is C.c_int and len(argtypes) == 16
    assert argtypes == sm[:7] + sm[8:]                                           # aft_link_sm_f32's list without reg
    assert argtypes[0]._type_ is _abi.AftLink and [i for i, t in enumerate(argtypes) if t is C.c_int] == [8, 9, 10, 14]
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_joint_f32") == names.index("aft_link_sm_f32") + 1
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "adafortitran_amd.h")).read()
    declared = re.findall(r"^(?:int|size_t|const char \*)\s*(aft_\w+)\(", header, flags=re.M)
    assert declared.index("aft_link_joint_f32") == declared.index("aft_link_sm_f32") + 1          # the header's order


def joint_flagged_shares(cfg, flags):
    """(share of the data (element, stream, bit) triples flagged, share of the data (element, stream) pairs with any flagged bit)."""
    pairs = cfg.data_elements * flags.shape[0] * flags.shape[1]
    if not pairs:
        return 0.0, 0.0
    return float(flags.sum()) / (pairs * cfg.bits_per_symbol), float(flags.any(axis=-1).sum()) / pairs


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_flagged_shares_on_the_inputs_the_gpu_tests_use(m):
    """At most 4e-2 of the data (element, stream, bit) triples and 1.5e-1 of the (element, stream) pairs at the derived tau(R), for
    every grid, R and estimate.  Measured with the float64 definition at tau = TAU_CAP >= tau(R) (the share is monotone in tau): at
    most 3.22e-2 and 1.17e-1, both on the default grid at R = 2, m = 8 with the ideal estimate."""
    worst_bits, worst_elems = (0.0, None), (0.0, None)
    for name, R, _ in sm_cases():
        for which in ("lmmse", "ideal"):
            sim, n, keys, sigma, ideal, est, rho, scale = _operands(name, R, which)
            cfg = LinkConfig(sim, m)
            flags = link_joint_host(cfg, keys, ideal, est, sigma, rho, scale, R, tau=derived_tau_joint(R))[4]
            bits, elems = joint_flagged_shares(cfg, flags)
            assert bits <= SM_SHARE_CAP and elems <= JOINT_ELEMENT_SHARE_CAP, (name, R, which, bits, elems)
            worst_bits, worst_elems = max(worst_bits, (bits, (name, R, which))), max(worst_elems, (elems, (name, R, which)))
    print(f"m = {m}: the largest flagged shares at tau(R) are {worst_bits[0]:.2e} of the bits at {worst_bits[1]} and "
          f"{worst_elems[0]:.2e} of the elements at {worst_elems[1]}")
