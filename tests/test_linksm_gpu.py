"""``aft_link_sm_f32``, ``hip_ops.LinkSmPlan`` and the ``streams=`` / ``detector=`` arguments of the accumulators and sweeps on the HIP
device: the kernel's counts, LLRs and losses against the float64 definition (``linksim.link_sm_host``) through the bounds derived below,
an unheard second stream against the diversity kernel bit for bit, independence of the batch, of the position and of the run, no
unwritten element, the 8- and 4-byte forms, the checked build, the refusals, the coded accumulators against the host decoders on the
device's own LLRs, and the physical orderings.

The shapes are tests/test_linksm.py's ``sm_inputs``: seed 3, frames 0..15 of the default grid (16-byte loads, 840 pairs over 256
threads), 0..31 of 30 x 7 (odd T: 8-byte loads, a ragged last pass) and the four frames of 3 x 5 (an odd number of elements whose
last is data, alone in its pair), each frame at the SNR it was drawn with, so the weights are mixed; R in (2, 3, 4, 8) on the frames
whole groups of 2 R fill; ZF and MMSE; the LMMSE estimate and the channel itself.

The bounds (``test_linksm.derived_tau`` / ``derived_e_lambda``) follow the kernel's operation chain as tests/test_linksim_gpu.py and
tests/test_linkmrc_gpu.py follow theirs (u = 2^-24, every float32 operation errs by at most u times its result, no fast-math; ``rho``,
``scale`` and ``reg`` are the same float32 numbers on both sides).  Complex quantities carry a bound on the MAGNITUDE of their error,
which also bounds each component; a rounding of both components of a complex number z is at most u |z| in magnitude:

* x, H x and the noise radius as in tests/test_linksim_gpu.py: e_x = (1+u)^2 - 1, e_h = (1 + e_x)(1 + u)^2 - 1 (about 4 u) of
  |H||x|, the radius within e_r (about 10 u); a component of exp(j 2 pi u2) is within 8 u, the pair within sqrt(2) 8 u:
  e_n = e_r + sqrt(2) 8 u (1 + e_r) (about 21 u) of |noise|.
* the two-term sample: stream 0's product as before, stream 1's two products enter by one fused multiply-add each (the product
  exact inside it, the partial sum rounds), the noise by one more: three roundings of partial sums that are within the partial reach:
  e_y = (1 + max(e_h, e_n))(1 + u)^3 - 1 (about 24 u) of reach(y_r) = |H_r0||x_0| + |H_r1||x_1| + |noise_r|.
* y conj(E_rs): a product and a fused multiply-add per component: e_c1 = e_y + 2 u (1 + e_y) of reach(y_r) |E_rs|.
* m_s = fma(rho_r, ., m_s), R of them: e_m(R) = (1 + e_c1)(1 + u)^R - 1 (about 34 u at R = 8) of reach(m_s).
* g00, g11: sums of non-negative terms, two roundings a term and one a branch: e_g(R) = (1 + u)^(2 + R) - 1; g01 likewise, of
  G01 = sum_r rho_r |E_r0||E_r1|, as a magnitude.  a = g + reg rounds once: e_a(R) = (1 + e_g)(1 + u) - 1.
* the adjugate: gx m_other is a product and a fused multiply-add per component of two perturbed factors:
  e_t = (1 + e_g)(1 + e_m)(1 + 2 u) - 1 of G01 reach(m_other); a_other m_self carries (1 + e_a)(1 + e_m) - 1 of a_other reach(m_self);
  the subtraction is the last fused multiply-add's one rounding:  e_c(R) = (1 + max(., e_t))(1 + u) - 1 (about 47 u at R = 8) of
  reach(c_s) = a_other reach(m_self) + G01 reach(m_other).
* p_s = fma(g_self, a_other, -|g01|^2): |g01|^2 within (1 + e_g)^2 (1 + u)^2 - 1 of G01^2, g_self a_other within (1 + e_g)(1 + e_a) - 1,
  one rounding: e_p(R) (about 23 u at R = 8) of P_s = g_self a_other + G01^2; the threshold beta_b p_s adds the three roundings
  of tests/test_linksim_gpu.py (2 d, the product with p, the product with the integer).

tau(R) = max(e_c(R), (1 + e_p(R))(1 + u)^3 - 1): 2.8e-6 at R = 8.  e_lambda(R) is tests/test_linksoft_gpu.py's chain with e_c(R) and
e_p(R) in place of its e_c and e_p, and eff_s = scale / a_other (a_other within e_a, ONE correctly rounded division: one more u) in
place of the exact scale: e_lambda = (1 + e_eff)(1 + u)(2 + e_d) - 2 with e_eff = (1 + u) / (1 - e_a) - 1: 7.8e-6 at R = 8.  Both are
below TAU_CAP = 1e-5.  The cancellation in p_s makes the margin's denominator (sums of absolute values) far larger than |p_s| where
the estimated channel is nearly singular, so more decisions are flagged than on the one-stream links: at most 4e-2 of the data
(element, axis, stream) triples (tests/test_linksm.py).  The loss is compared as tests/test_linksoft_gpu.py compares it
(``derived_e_s``: the softplus terms and the order of a stream's sums are the soft kernel's).

Measured on one MI355X (the figures this file prints): see the table in DESIGN.md, "Spatial multiplexing on the link"."""
import numpy as np
import pytest
import torch

import link2_gpu
from adafortitran_amd import _abi, ingest
from adafortitran_amd.chansim import ChannelSimConfig, ls_interpolate, make_pack
from adafortitran_amd.hip_ops import LinkMrcPlan
from adafortitran_amd.linksim import BITS_PER_SYMBOL, DETECTORS, LinkConfig, link_sm_host
from adafortitran_amd.lmmse import LmmseEstimator
from link2_gpu import DEV, FACTORS, operands as _operands, plan as _plan, run as _run
from test_linksim import TAU_CAP
from test_linksim_gpu import _dev
from test_linksm import SM_SHARE_CAP, derived_e_lambda, derived_tau, sm_cases, sm_flagged_share, sm_inputs
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    assert derived_tau(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


_wants = {}


def _want(name, m, R, which, detector):
    """The definition at tau(R) and e_lambda(R), computed once and flattened to G N rows: (counts, loss, llr, wrong, flags, loss_lo,
    loss_hi, q)."""
    if (name, m, R, which, detector) not in _wants:
        _, (ideal, est, keys, sigma, rho, scale, reg), _ = _operands(detector, name, R, which)
        out = link_sm_host(LinkConfig(sm_inputs(name)[0], m), keys, ideal, est, sigma, rho, scale, reg, R, 2, FACTORS,
                           tau=derived_tau(R), e_lambda=derived_e_lambda(R))
        _wants[name, m, R, which, detector] = (out[4],) + tuple(v.reshape(-1, *v.shape[2:]) for v in out)
    return _wants[name, m, R, which, detector]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    rows = with_flags = differing = 0
    worst_llr = worst_share = 0.0
    for name, R, n in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        e_s, e_l = derived_e_s(cfg), derived_e_lambda(R)
        for detector in DETECTORS:
            for which in ("lmmse", "ideal"):
                flags5, want_counts, _, want_llr, _, flags, lo, hi, q = _want(name, m, R, which, detector)
                counts, loss, llr = _run(detector, name, m, R, which)
                F = n // R                                                     # G N rows
                assert counts.shape == (F, 2) and counts.dtype == torch.int32 and loss.shape == (F, 3) and llr.shape == (F, *cfg.sim.ofdm, m)
                share = sm_flagged_share(cfg, flags5)
                assert share <= SM_SHARE_CAP, (name, R, detector, which, share)
                got = counts.cpu().numpy().astype(np.int64)
                triples, elems = flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2))
                assert (got >= 0).all() and (np.abs(got[:, 0] - want_counts[:, 0]) <= triples).all(), (name, R, detector, which, got, want_counts, triples)
                assert (np.abs(got[:, 1] - want_counts[:, 1]) <= elems).all(), (name, R, detector, which, got, want_counts, elems)
                got_llr = llr.cpu().numpy().astype(np.float64)
                err = np.abs(got_llr - want_llr)
                assert np.isfinite(got_llr).all() and (err <= e_l * q).all(), (name, R, detector, which, float((err / np.where(q > 0, q, 1)).max()))
                got_loss = loss.cpu().numpy().astype(np.float64)
                assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all(), \
                    (name, R, detector, which, got_loss, lo, hi)
                rows += F
                with_flags += int((triples > 0).sum())
                differing += int((got != want_counts).any(axis=1).sum())
                worst_llr = max(worst_llr, float((err[q > 0] / q[q > 0] / e_l).max()))
                worst_share = max(worst_share, share)
    print(f"m = {m}: {with_flags} of {rows} (group, stream) rows had a flagged decision at tau(R); {differing} differ from the definition; "
          f"largest flagged share {worst_share:.2e}; largest |llr_dev - llr_def| / (e_lambda(R) q) = {worst_llr:.2f}")


def _unheard(name, R):
    """``_operands`` with ``H_r1 = E_r1 = 0``, scale 4 and reg 0.25, on the device, and the diversity link's operands on the frames (r, 0)."""
    n, (ideal, est, keys, sigma, rho, _, _), _ = _operands("mmse", name, R)
    G = n // (2 * R)
    H, E = ideal.copy(), est.copy()
    H[1::2], E[1::2] = 0, 0
    scale, reg = np.full(G, 4.0, np.float32), np.full(G, 0.25, np.float32)
    sm = tuple(_dev(a) for a in (H, E, keys, sigma, rho, scale, reg))
    mrc = tuple(_dev(np.ascontiguousarray(a)) for a in (ideal[::2], est[::2], keys[::2], sigma[::2], rho[::2], scale))
    return G, sm, mrc


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_stream_is_the_diversity_kernel_bit_for_bit(m):
    """The reason for keeping ``link_walk``'s thread map, fused multiply-add chains and reduction order: with ``H_r1 = E_r1 = 0``,
    ``scale = 4`` and ``reg = 0.25`` stream 0's counts, LLRs and losses are ``LinkMrcPlan``'s on the frames (r, 0)."""
    f = _dev(FACTORS)
    for name, R, _ in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        G, sm, mrc = _unheard(name, R)
        counts, loss, llr = _plan("mmse", name, m, R)(*sm, f, want_llr=True)
        want = LinkMrcPlan(cfg, DEV, R)(*mrc, f, want_llr=True)
        for got, w in zip((counts, loss, llr), want):
            assert torch.equal(got.view(G, 2, *got.shape[1:])[:, 0], w), (name, R)
        assert (llr.view(G, 2, *llr.shape[1:])[:, 1] == 0).all()                  # c_1 = p_1 = 0: the unheard stream's LLRs


# ---- what both two-stream entry points are asked alike: the bodies are link2_gpu's ----

@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    link2_gpu.group_independence(m, ((2, "mmse"), (3, "zf")))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_a_null_llr_and_bases_off_16_bytes(m):
    link2_gpu.poisoned_outputs("mmse", m)


def test_checked_build_gives_the_same_bits():
    link2_gpu.checked_build(((2, "mmse"), (3, "zf"), (8, "mmse")))


def test_what_the_plan_refuses():
    link2_gpu.plan_refusals("mmse")


def test_every_refusal_of_the_entry_point_launches_nothing():
    link2_gpu.entry_refusals("mmse")


@pytest.mark.parametrize("kind", ("viterbi", "ldpc"))
def test_coded_accumulators_with_two_streams_run_without_a_synchronisation(kind):
    link2_gpu.coded_accumulators(kind, "mmse")


class _Ls(torch.nn.Module):
    """The LS-interpolated estimate as a model ``evaluation.forward_pass`` can call."""

    def __init__(self, sim):
        super().__init__()
        self.sim = sim
        self.register_buffer("anchor", torch.zeros(1))

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.cpu().numpy())).to(pilots.device)


def test_physical_orderings_on_the_device():
    """Recorded and printed; asserted is the ordering only.  One simulated pack of 64 frames at 15 dB, 16-QAM.  The 1 x R diversity
    link beside it runs on the same frames, R at a time."""
    from adafortitran_amd.evaluation import get_link_rates, get_link_stats
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    pack = make_pack(sim, 64, seed=31, snr_db=15.0)
    loaders = [("SNR_15", ingest.ResidentLoader(pack, sim.pilot, 32, device=DEV, shuffle=False))]
    models = {"perfect": None, "lmmse": LmmseEstimator(sim).to(DEV), "ls": _Ls(sim).to(DEV)}
    ber = {(R, d): {name: get_link_stats(model, loaders, cfg, seed=1, branches=R, streams=2, detector=d)[15] for name, model in models.items()}
           for R in (2, 4, 8) for d in DETECTORS}
    one = {R: get_link_stats(models["lmmse"], loaders, cfg, seed=1, branches=R)[15] for R in (2, 4, 8)}
    gmi = {(R, d): get_link_rates(models["lmmse"], loaders, cfg, seed=1, branches=R, streams=2, detector=d)[15] for R in (2, 4) for d in DETECTORS}
    print("BER per (antennas, detector) and estimator:", ber, " 1 x R with the LMMSE estimate:", one, " GMI per stream, LMMSE:", gmi)
    for d in DETECTORS:
        assert all(ber[2, d][w] > ber[4, d][w] > ber[8, d][w] for w in models)                 # BER falls with R
        assert all(ber[R, d]["perfect"] <= ber[R, d]["lmmse"] <= ber[R, d]["ls"] for R in (2, 4, 8))
        assert all(ber[R, d]["lmmse"] >= one[R] for R in (2, 4, 8))
    assert all(ber[2, "mmse"][w] <= ber[2, "zf"][w] for w in models)
    assert all(0 < v <= 4 for v in gmi.values()) and gmi[4, "mmse"] >= gmi[2, "mmse"]
