"""``aft_link_joint_f32``, ``hip_ops.LinkJointPlan`` and ``detector="joint"`` on the accumulators and sweeps on the HIP device: the kernel's
counts, LLRs and losses against the float64 definition (``linksim.link_joint_host``) through the bounds derived below, an unheard second
stream, independence of the batch, of the position and of the run, no unwritten element, the 8- and 4-byte forms, the checked build,
the refusals, the coded accumulators against the host decoders on the device's own LLRs, and the physical orderings beside MMSE.

The shapes are tests/test_linksm.py's ``sm_inputs`` and ``sm_cases``: 16 frames of 120 x 14, 32 of 30 x 7 and the four frames of 3 x 5, R
in (2, 3, 4, 8) on the frames whole groups of 2 R fill, the LMMSE estimate and the channel itself.

The bounds (``test_linkjoint.derived_tau_joint`` / ``derived_e_lambda_joint``) follow the kernel's operation chain (csrc/link_device.h,
``link_joint_llrs``) as tests/test_linksm_gpu.py follows its own: u = 2^-24, every float32 operation errs by at most u times its result,
no fast-math, nothing contracted behind the source; ``rho`` and ``scale`` are the same float32 numbers on both sides.  A complex quantity
carries a bound on the MAGNITUDE of its error; its two components then sum to at most sqrt(2) times it.  Every error is written in
units of the SHARE of ``Q = 2 A^2 (g00 + g11 + 2 G01) + 2 sqrt(2) A (reach(m_0) + reach(m_1))`` that bounds the term (``linksim``, "the
joint link"), so the errors of a candidate's terms add up to a multiple of ``Q``:

* the operands, from tests/test_linksm_gpu.py: ``m_s`` within e_m(R) of reach(m_s) (about 34 u at R = 8), ``g00`` / ``g11`` within
  e_g(R) = (1+u)^(2+R) - 1 of themselves and ``g01`` within e_g(R) of G01; a level ``a_k = d (2 k - (L-1))`` within e_a = (1+u)^2 - 1
  (d rounds once, the product once; the integer is exact).
* the stream's own terms, per axis ``t(k) = a_k fma(a_k, g_ee, -2 comp)``: the piece ``a_k^2 g_ee`` carries two levels, the sum and two
  roundings, e_p = (1+e_a)^2 (1+e_g) (1+u)^2 - 1 of ``A^2 g_ee``; the piece ``2 a_k comp`` one level, the component and the same two
  roundings.  Over both axes the components sum to at most sqrt(2) reach(m_e) and their errors to sqrt(2) e_m reach(m_e), so
  e_t = max(e_p, (1+e_a)(1+e_m)(1+u)^2 - 1) of the share ``2 A^2 g_ee + 2 sqrt(2) A reach(m_e)``.
* ``z = m_o - g_oe x_e``, two fused multiply-adds per component (the products exact inside them), whose partial sums stay within
  ``Z = reach(m_o) + sqrt(2) A G01``: e_z = (1 + max(e_m, (1+e_g)(1+e_a) - 1))(1+u)^2 - 1 of Z, as a magnitude.
* the inner minimum, per axis ``min_i fma(-2 a_i, |comp z|, a_i^2 g_oo)`` over the positive levels.  In exact arithmetic it is
  ``min_k mu_k``: the mirrored level's metric is larger by ``4 a_i |comp|``.  ``a_i^2 g_oo = (a_i a_i) g_oo`` is within e_p of ``A^2 g_oo``,
  ``-2 a_i`` is exact in ``a_i``, the fused multiply-add rounds once; a minimum of perturbed metrics moves by at most the largest
  perturbation.  Over both axes: e_r = max((1+e_p)(1+u) - 1, (1+e_a)(1+u)(1+e_z) - 1) of the share ``2 A^2 g_oo + 2 sqrt(2) A Z``
  ``= 2 A^2 g_oo + 2 sqrt(2) A reach(m_o) + 4 A^2 G01``.
* ``f = (t(ki) + t(kq)) + (r_I + r_Q)``: every term passes two additions: e_f(R) = (1 + max(e_t, e_r))(1+u)^2 - 1 of Q, about 41 u at
  R = 8.

A bit's two minima each move by at most e_f Q and their difference rounds once, ``|min1 - min0| <= 2 Q (1 + e_f)``:
tau(R) = 2 e_f + 2 u (1 + e_f), 5.0e-6 at R = 8.  ``Lambda_j = scale Delta_j`` rounds once more: e_lambda(R) = tau + u (2 + tau), 5.2e-6
at R = 8.  Both are below TAU_CAP = 1e-5.  A device decision is the sign of the device's own LLR, so it can differ from the
definition's only on a flagged bit: the counts are compared through the flagged bits and elements of each row, whose shares
tests/test_linkjoint.py caps.  The loss is compared as tests/test_linksoft_gpu.py compares it (``derived_e_s``: the softplus terms and
the order of a stream's sums are the soft kernel's).

Measured on one MI355X (the figures this file prints): see the table in DESIGN.md, "Joint detection on the link"."""
from functools import partial

import numpy as np
import pytest
import torch

import link2_gpu
from adafortitran_amd import _abi, ingest
from adafortitran_amd.chansim import ChannelSimConfig, make_pack
from adafortitran_amd.linksim import BITS_PER_SYMBOL, JOINT_DETECTOR, LinkConfig, link_joint_host, link_mrc_host
from adafortitran_amd.lmmse import LmmseEstimator
from link2_gpu import DEV, FACTORS
from test_linkjoint import JOINT_ELEMENT_SHARE_CAP, derived_e_lambda_joint, derived_tau_joint, joint_flagged_shares
from test_linksim import TAU_CAP
from test_linksim_gpu import _dev
from test_linksm import SM_SHARE_CAP, sm_cases, sm_inputs
from test_linksm_gpu import _Ls
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
_plan, _operands, _run = (partial(fn, JOINT_DETECTOR) for fn in (link2_gpu.plan, link2_gpu.operands, link2_gpu.run))


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    assert derived_tau_joint(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda_joint(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


_wants = {}


def _want(name, m, R, which):
    """The definition at tau(R) and e_lambda(R), computed once and flattened to G N rows: (counts, loss, llr, wrong, flags, loss_lo,
    loss_hi, q), and the flags unflattened first."""
    if (name, m, R, which) not in _wants:
        _, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R, which)
        out = link_joint_host(LinkConfig(sm_inputs(name)[0], m), keys, ideal, est, sigma, rho, scale, R, 2, FACTORS,
                              tau=derived_tau_joint(R), e_lambda=derived_e_lambda_joint(R))
        _wants[name, m, R, which] = (out[4],) + tuple(v.reshape(-1, *v.shape[2:]) for v in out)
    return _wants[name, m, R, which]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    rows = with_flags = differing = 0
    worst_llr = worst_bits = worst_elems = 0.0
    for name, R, n in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        e_s, e_l = derived_e_s(cfg), derived_e_lambda_joint(R)
        for which in ("lmmse", "ideal"):
            flags5, want_counts, _, want_llr, _, flags, lo, hi, q = _want(name, m, R, which)
            counts, loss, llr = _run(name, m, R, which)
            F = n // R                                                         # G N rows
            assert counts.shape == (F, 2) and counts.dtype == torch.int32 and loss.shape == (F, 3) and llr.shape == (F, *cfg.sim.ofdm, m)
            bits, elems = joint_flagged_shares(cfg, flags5)
            assert bits <= SM_SHARE_CAP and elems <= JOINT_ELEMENT_SHARE_CAP, (name, R, which, bits, elems)
            got = counts.cpu().numpy().astype(np.int64)
            flagged_bits, flagged_elems = flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2))
            assert (got >= 0).all() and (np.abs(got[:, 0] - want_counts[:, 0]) <= flagged_bits).all(), (name, R, which, got, want_counts, flagged_bits)
            assert (np.abs(got[:, 1] - want_counts[:, 1]) <= flagged_elems).all(), (name, R, which, got, want_counts, flagged_elems)
            got_llr = llr.cpu().numpy().astype(np.float64)
            err = np.abs(got_llr - want_llr)
            ratio = float((err[q > 0] / q[q > 0] / e_l).max())
            print(f"m = {m}, {name}, R = {R}, {which}: largest |llr_dev - llr_def| / (e_lambda(R) q) = {ratio:.3f}; flagged shares {bits:.2e} of "
                  f"the bits, {elems:.2e} of the elements; rows that differ {int((got != want_counts).any(axis=1).sum())} of {F}")
            assert np.isfinite(got_llr).all() and (err <= e_l * q).all(), (name, R, which, ratio)
            got_loss = loss.cpu().numpy().astype(np.float64)
            assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all(), \
                (name, R, which, got_loss, lo, hi)
            rows += F
            with_flags += int((flagged_bits > 0).sum())
            differing += int((got != want_counts).any(axis=1).sum())
            worst_llr, worst_bits, worst_elems = max(worst_llr, ratio), max(worst_bits, bits), max(worst_elems, elems)
    print(f"m = {m}: {with_flags} of {rows} (group, stream) rows had a flagged bit at tau(R); {differing} differ from the definition; largest "
          f"flagged shares {worst_bits:.2e} (bits) and {worst_elems:.2e} (elements); largest |llr_dev - llr_def| / (e_lambda(R) q) = {worst_llr:.3f}")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_stream(m):
    """``H_r1 = E_r1 = 0``: every candidate of stream 1 has the same metric, so its LLRs are exactly 0 on the device; stream 0's are
    within e_lambda(R) q of ``link_mrc_host``'s on the frames (r, 0), which the definition equals there."""
    f = _dev(FACTORS)
    for name, R, _ in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        n, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R)
        G = n // (2 * R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        counts, loss, llr = _plan(name, m, R)(*(_dev(a) for a in (H, E, keys, sigma, rho, scale)), f, want_llr=True)
        llr = llr.view(G, 2, *llr.shape[1:])
        assert (llr[:, 1] == 0).all(), (name, R)
        q = link_joint_host(cfg, keys, H, E, sigma, rho, scale, R, e_lambda=0.0)[5]
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R)[2]
        err = np.abs(llr[:, 0].cpu().numpy().astype(np.float64) - want)
        assert (err <= derived_e_lambda_joint(R) * q[:, 0]).all(), (name, R, float((err / np.where(q[:, 0] > 0, q[:, 0], 1)).max()))
        np.testing.assert_allclose(loss.view(G, 2, -1)[:, 1, 0].cpu().numpy(), m * cfg.data_elements, rtol=1e-5)


def test_all_zero_estimates_give_zero_llrs():
    for m in BITS_PER_SYMBOL:
        _, _, (h, e, k, s, rho, c) = _operands("odd_30x7", 2)
        counts, loss, llr = _plan("odd_30x7", m, 2)(h, torch.zeros_like(e), k, s, rho, c, _dev(FACTORS), want_llr=True)
        assert (llr == 0).all() and loss.isfinite().all() and (counts >= 0).all()


# ---- what both two-stream entry points are asked alike: the bodies are link2_gpu's ----

@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    link2_gpu.group_independence(m, ((2, JOINT_DETECTOR), (3, JOINT_DETECTOR)))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_a_null_llr_and_bases_off_16_bytes(m):
    link2_gpu.poisoned_outputs(JOINT_DETECTOR, m)


def test_checked_build_gives_the_same_bits():
    link2_gpu.checked_build(((2, JOINT_DETECTOR), (3, JOINT_DETECTOR), (8, JOINT_DETECTOR)))


def test_what_the_plan_refuses():
    link2_gpu.plan_refusals(JOINT_DETECTOR)


def test_every_refusal_of_the_entry_point_launches_nothing():
    link2_gpu.entry_refusals(JOINT_DETECTOR)


@pytest.mark.parametrize("kind", ("viterbi", "ldpc"))
def test_coded_accumulators_with_the_joint_detector_run_without_a_synchronisation(kind):
    link2_gpu.coded_accumulators(kind, JOINT_DETECTOR)


def test_physical_orderings_on_the_device():
    """Recorded and printed; asserted is the ordering only.  One simulated pack of 64 frames at 15 dB, 16-QAM."""
    from adafortitran_amd.evaluation import get_link_rates, get_link_stats
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    pack = make_pack(sim, 64, seed=31, snr_db=15.0)
    loaders = [("SNR_15", ingest.ResidentLoader(pack, sim.pilot, 32, device=DEV, shuffle=False))]
    models = {"perfect": None, "lmmse": LmmseEstimator(sim).to(DEV), "ls": _Ls(sim).to(DEV)}
    ber = {(R, d): {name: get_link_stats(model, loaders, cfg, seed=1, branches=R, streams=2, detector=d)[15] for name, model in models.items()}
           for R in (2, 4, 8) for d in ("mmse", "joint")}
    gmi = {(R, d): {name: get_link_rates(models[name], loaders, cfg, seed=1, branches=R, streams=2, detector=d)[15] for name in ("perfect", "lmmse")}
           for R in (2, 8) for d in ("mmse", "joint")}
    print("BER per (antennas, detector) and estimator:", ber, " GMI per stream:", gmi)
    print("LS, joint against MMSE:", {R: (ber[R, "joint"]["ls"], ber[R, "mmse"]["ls"]) for R in (2, 4, 8)},
          " R = 8, joint against MMSE:", {w: (ber[8, "joint"][w], ber[8, "mmse"][w]) for w in models})
    for w in ("perfect", "lmmse"):
        assert ber[2, "joint"][w] <= ber[2, "mmse"][w] and gmi[2, "joint"][w] >= gmi[2, "mmse"][w]
    assert all(ber[2, "joint"][w] > ber[4, "joint"][w] > ber[8, "joint"][w] for w in models)           # BER falls with R
    assert all(ber[R, "joint"]["perfect"] <= ber[R, "joint"]["lmmse"] <= ber[R, "joint"]["ls"] for R in (2, 4, 8))
