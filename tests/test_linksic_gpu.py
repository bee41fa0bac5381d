"""``aft_link_sic_f32``, ``hip_ops.LinkSicPlan`` and ``detector="sic"`` on the HIP device: the kernel's counts, LLRs, losses and three
integers against the float64 definition (``linksim.link_sic_host``) through the bounds derived below, the first-detected stream against
the linear kernel bit for bit, a tie, an unheard second stream against the diversity kernel bit for bit, independence of the batch, of
the position and of the run, no unwritten element with a NULL ``llr`` and a NULL ``stats`` and bases off 16 bytes, the checked build,
the refusals, the coded accumulators against the host decoders on the device's own LLRs, and ``sic_propagation`` of a device sweep.

The shapes are tests/test_linksm.py's ``sm_inputs`` (tests/test_linksm_gpu.py describes them): the default grid (16-byte loads), 30 x 7
(8-byte loads, a ragged last pass) and 3 x 5 (an odd element count whose last element is data), each frame at its own SNR, R in
(2, 3, 4, 8) on the frames whole groups fill, the LMMSE estimate and the channel itself; ``reg`` is the MMSE one.

The bounds (``test_linksic.derived_tau_sic`` / ``derived_e_lambda_sic``; u = 2^-24, every float32 operation errs by at most u times its
result, complex quantities carry a bound on the MAGNITUDE of their error as in tests/test_linksm_gpu.py):

* first stage: the linear kernel's chain, call for call: ``test_linksm.derived_tau`` / ``derived_e_lambda``.
* second stage, at an element that is not dependent -- the order and the first decision are then the definition's, so x^ is the same
  level on both sides --: x^ = d (2 k - (L - 1)) is float32(d) times an exact integer, e_x = (1 + u)^2 - 1 of |x^|; m_o is within
  e_m(R) of reach(m_o) and g01 within e_g(R) = (1 + u)^(2 + R) - 1 of G01 (tests/test_linksm_gpu.py).  A component of c_o is two fused
  multiply-adds: the products of the perturbed g01 and x^ are exact inside them, within (1 + e_g)(1 + e_x) - 1 of G01 |x^| together,
  and each rounds a partial sum that is within the partial reach:
  e_c2(R) = (1 + max(e_m(R), (1 + e_g)(1 + e_x) - 1))(1 + u)^2 - 1 (36.3 u at R = 8) of reach(c_o) = reach(m_o) + G01 |x^|.
* p_o = g_oo is within e_g(R) of itself (a sum of non-negative terms); the threshold beta_b p_o adds the three roundings of
  tests/test_linksim_gpu.py.  The order g11 > g00 can differ only where |g00 - g11| <= e_g (g00 + g11).

tau_sic(R) = max(tau(R), e_c2(R), (1 + e_g(R))(1 + u)^3 - 1) = tau(R): 47.3 u = 2.8e-6 at R = 8, the adjugate's chain stays the longest.
e_lambda_sic(R) is the larger of e_lambda(R) and tests/test_linksoft_gpu.py's chain with e_c2(R) and e_g(R) in place of its e_c and
e_p at the exact ``scale``: 130.6 u = 7.8e-6 at R = 8.  Both are below TAU_CAP = 1e-5.  The loss is compared as
tests/test_linksoft_gpu.py compares it (``derived_e_s``: a stream's softplus terms enter its sums in the linear kernel's order).

What a dependent element allows (``linksim``, "the successive-cancellation link"): m bits and 1 symbol on the second stream's row, LLRs
within 2 q_dep; the third integer (first decision wrong AND the other stream wrong) may also move where the second stream's own
decision is flagged.

Measured on one MI355X (the figures this file prints): see the table in DESIGN.md, "Successive cancellation on the link"."""
import ctypes
import os

import numpy as np
import pytest
import torch

import link2_gpu
from adafortitran_amd import _abi, _lib, linksim
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkMrcPlan, LinkSicPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, BlockErrorAccumulator, CodeConfig, LdpcBlockErrorAccumulator, LdpcConfig,
                                      LinkAccumulator, LinkConfig, link_decode_host, link_ldpc_host, noise_sigma, sm_weights)
from adafortitran_amd.lmmse import LmmseEstimator
from link2_gpu import DEV, FACTORS, POISON
from test_chansim_gpu import _no_sync, _same_bits
from test_linkmrc import MRC_ODD
from test_linksic import DEPENDENT_CAP, _order, derived_e_lambda_sic, derived_tau_sic, sic_shares
from test_linksim import TAU_CAP
from test_linksim_gpu import _dev
from test_linksm import SM_SHARE_CAP, sm_cases, sm_inputs
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
_plans, _wants = {}, {}


def _operands(name, R, which="lmmse"):
    """(n, host operands, device operands): ``link2_gpu``'s for the MMSE detector -- (ideal, est, keys, sigma, rho, scale, reg)."""
    return link2_gpu.operands("mmse", name, R, which)


def _plan(name, m, R):
    if (name, m, R) not in _plans:
        _plans[name, m, R] = LinkSicPlan(LinkConfig(sm_inputs(name)[0], m), DEV, R)
    return _plans[name, m, R]


def _run(name, m, R, which="lmmse", want_llr=True, lib=None):
    return _plan(name, m, R)(*_operands(name, R, which)[2], _dev(FACTORS), want_llr=want_llr, lib=lib)


def _entry(plan, ops, factors, counts, loss, llr, stats, batch, hp=None, ep=None):
    h, e, *rest = ops
    return _lib.load().aft_link_sic_f32(
        ctypes.byref(plan.link), hp or h.data_ptr(), ep or e.data_ptr(), *(t.data_ptr() for t in rest), factors.data_ptr(), factors.numel(),
        plan.branches, plan.streams, counts.data_ptr(), loss.data_ptr(), llr, stats, batch, _lib.current_stream_ptr(counts.device))


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    assert derived_tau_sic(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda_sic(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


def _want(name, m, R, which):
    """The definition at tau_sic(R) and e_lambda_sic(R), computed once: ``link_sic_host``'s tuple and the order f [G, S, T]."""
    if (name, m, R, which) not in _wants:
        _, (ideal, est, keys, sigma, rho, scale, reg), _ = _operands(name, R, which)
        sim = sm_inputs(name)[0]
        out = linksim.link_sic_host(LinkConfig(sim, m), keys, ideal, est, sigma, rho, scale, reg, R, 2, FACTORS,
                                    tau=derived_tau_sic(R), e_lambda=derived_e_lambda_sic(R))
        _wants[name, m, R, which] = (out, _order(est, rho, R, sim.ofdm))
    return _wants[name, m, R, which]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    worst = dict(llr=0.0, free=0.0, bits=0.0, dependent=0.0, flagged=0.0)
    rows = differing = 0
    for name, R, n in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        e_s, e_l = derived_e_s(cfg), derived_e_lambda_sic(R)
        for which in ("lmmse", "ideal"):
            (want_counts, _, want_llr, want_stats, _, flags, dep, lo, hi, q), f = _want(name, m, R, which)
            counts, loss, llr, stats = _run(name, m, R, which)
            G = n // (2 * R)
            assert counts.shape == (2 * G, 2) and counts.dtype == torch.int32 and loss.shape == (2 * G, 3)
            assert llr.shape == (2 * G, *cfg.sim.ofdm, m) and stats.shape == (G, 3) and stats.dtype == torch.int32
            shares = sic_shares(cfg, (None,) * 5 + (flags, dep), f)
            assert shares[0] <= DEPENDENT_CAP and shares[1] <= SM_SHARE_CAP, (name, R, which, shares)
            second = np.stack([f, ~f], axis=1)                                   # [G, N, S, T]: stream s is the second-detected one
            free = ((dep > 0)[:, None] & second) | (dep == 2)[:, None]            # this (element, stream)'s outputs may differ freely
            got = counts.cpu().numpy().astype(np.int64).reshape(G, 2, 2)
            triples, elems, loose = flags.sum(axis=(2, 3, 4)), flags.any(axis=4).sum(axis=(2, 3)), free.sum(axis=(2, 3))
            assert (got >= 0).all() and (np.abs(got[..., 0] - want_counts[..., 0]) <= triples + m * loose).all(), (name, R, which)
            assert (np.abs(got[..., 1] - want_counts[..., 1]) <= elems + loose).all(), (name, R, which)
            got_llr = llr.cpu().numpy().astype(np.float64).reshape(want_llr.shape)
            err, freeb = np.abs(got_llr - want_llr), np.broadcast_to(free[..., None], want_llr.shape)
            assert np.isfinite(got_llr).all() and (err <= e_l * q)[~freeb].all(), (name, R, which, float((err / np.where(q > 0, q, 1))[~freeb].max()))
            assert (np.abs(got_llr) <= 2 * q * (1 + e_l))[freeb].all(), (name, R, which)
            got_loss = loss.cpu().numpy().astype(np.float64).reshape(lo.shape)
            assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all(), \
                (name, R, which, got_loss, lo, hi)
            got_stats = stats.cpu().numpy().astype(np.int64)
            order, dependent = (dep == 2).sum(axis=(1, 2)), (dep > 0).sum(axis=(1, 2))
            own = (flags.any(axis=4) & second).any(axis=1).sum(axis=(1, 2))      # the second stream's own decision is flagged
            assert (np.abs(got_stats[:, 0] - want_stats[:, 0]) <= order).all(), (name, R, which, got_stats, want_stats)
            assert (np.abs(got_stats[:, 1] - want_stats[:, 1]) <= dependent).all(), (name, R, which, got_stats, want_stats)
            assert (np.abs(got_stats[:, 2] - want_stats[:, 2]) <= dependent + own).all(), (name, R, which, got_stats, want_stats)
            assert (got_stats >= 0).all() and (got_stats[:, 2] <= got_stats[:, 1]).all()
            rows += 2 * G
            differing += int((got != want_counts).any(axis=2).sum())
            keep = ~freeb & (q > 0)
            worst["llr"] = max(worst["llr"], float((err[keep] / q[keep] / e_l).max()))
            if freeb.any():
                worst["free"] = max(worst["free"], float((np.abs(got_llr)[freeb] / (2 * q[freeb])).max()))
            room = triples + m * loose
            worst["bits"] = max(worst["bits"], float((np.abs(got[..., 0] - want_counts[..., 0])[room > 0] / room[room > 0]).max(initial=0.0)))
            worst["dependent"], worst["flagged"] = max(worst["dependent"], shares[0]), max(worst["flagged"], shares[1])
    print(f"m = {m}: {differing} of {rows} (group, stream) rows differ from the definition; largest |llr_dev - llr_def| / (e_lambda_sic(R) q) = "
          f"{worst['llr']:.2f}; largest |llr_dev| / (2 q_dep) at dependent pairs = {worst['free']:.2f}; largest bit-count difference / its "
          f"allowance = {worst['bits']:.2f}; largest dependent share {worst['dependent']:.2e}, second stream's flagged share {worst['flagged']:.2e}")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_first_detected_stream_is_the_linear_kernel_bit_for_bit(m):
    """At every data element outside the definition's order-flagged set the first-detected stream's LLRs are ``aft_link_sm_f32``'s (MMSE)
    at that (element, stream): the first stage is the linear detector's calls."""
    for name, R, n in sm_cases():
        for which in ("lmmse", "ideal"):
            (_, _, _, _, _, _, dep, _, _, _), f = _want(name, m, R, which)
            mask = LinkConfig(sm_inputs(name)[0], m).data_mask
            first = np.stack([~f, f], axis=1) & (mask[None] & (dep != 2))[:, None]
            pick = _dev(first.reshape(-1, *first.shape[2:]))
            sic, sm = _run(name, m, R, which)[2], link2_gpu.run("mmse", name, m, R, which)[2]
            assert pick.sum().item() == int(mask.sum()) * len(f) - int((dep == 2).sum()) and torch.equal(sic[pick], sm[pick]), (name, R, which)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_tie_detects_stream_0_first_everywhere(m):
    """``E_r1 = conj(E_r0)``: ``g00 == g11`` bitwise, so stream 0 is the linear kernel's stream 0 whole and nothing is swapped."""
    f = _dev(FACTORS)
    for name, R, _ in sm_cases():
        n, (ideal, est, *rest), _ = _operands(name, R)
        E = est.copy()
        E[1::2] = E[0::2].conj()
        ops = tuple(_dev(a) for a in (ideal, E, *rest))
        counts, loss, llr, stats = _plan(name, m, R)(*ops, f, want_llr=True)
        want = link2_gpu.plan("mmse", name, m, R)(*ops, f, want_llr=True)
        for got, w in zip((counts, loss, llr), want):
            assert torch.equal(got[0::2], w[0::2]), (name, R)
        assert (stats[:, 0] == 0).all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_stream_is_the_diversity_kernel_bit_for_bit(m):
    """``H_r1 = E_r1 = 0``, ``scale = 4`` and ``reg = 0.25``: stream 0 is ``LinkMrcPlan`` on the frames (r, 0); stream 1's LLRs are 0."""
    f = _dev(FACTORS)
    for name, R, _ in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        n, (ideal, est, keys, sigma, rho, _, _), _ = _operands(name, R)
        G = n // (2 * R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        scale, reg = np.full(G, 4.0, np.float32), np.full(G, 0.25, np.float32)
        counts, loss, llr, stats = _plan(name, m, R)(*(_dev(a) for a in (H, E, keys, sigma, rho, scale, reg)), f, want_llr=True)
        want = LinkMrcPlan(cfg, DEV, R)(*(_dev(np.ascontiguousarray(a)) for a in (ideal[::2], est[::2], keys[::2], sigma[::2], rho[::2], scale)),
                                        f, want_llr=True)
        for got, w in zip((counts, loss, llr), want):
            assert torch.equal(got[0::2], w), (name, R)
        assert (llr[1::2] == 0).all() and (stats[:, 0] == 0).all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        sim, keys, sigma, snr, ideal, est = sm_inputs(name)
        for R in (2, 3):
            p, W = _plan(name, m, R), 2 * R
            idx = (np.arange(37 * W) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-W:] = np.arange(W, 2 * W)                                       # ... the last one group 1 of ``_operands``
            ops = lambda i: (_dev(ideal[i]), _dev(est["lmmse"][i]), _dev(keys[i]), _dev(sigma[i]),  # noqa: E731
                             *(_dev(a) for a in sm_weights(snr[i], 0.0, R, 2, "mmse")))
            batch = p(*ops(idx), f, want_llr=True)
            alone = p(*ops(np.arange(W, 2 * W)), f, want_llr=True)
            _same_bits([t[72:74] for t in batch[:3]] + [batch[3][36:37]], alone)
            whole = _run(name, m, R)
            _same_bits([t[2:4] for t in whole[:3]] + [whole[3][1:2]], alone)     # second of the groups of ``_operands``
            _same_bits(p(*ops(idx), f, want_llr=True), batch)                    # a second run of the same batch


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_null_llr_null_stats_and_bases_off_16_bytes(m):
    """Every element of the four outputs is written and nothing beside them; without the LLR output, without the stats, and with ideal,
    est and llr 8, 4 and 12 bytes off a 16-byte boundary, the same bits."""
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        for R in (2, 3):
            n, _, ops = _operands(name, R)
            p, F, G = _plan(name, m, R), n // R, n // (2 * R)
            want = _run(name, m, R)
            h, e = ops[0], ops[1]
            fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
            fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
            assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
            for hp, ep, off, with_stats in ((None, None, 0, True), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8, True), (None, fe.data_ptr() + 8, 0, False),
                                            (None, None, 8, False), (None, None, 4, True), (fh.data_ptr() + 8, None, 12, True),
                                            (None, None, None, True), (None, None, None, False)):
                counts = torch.full((F + 1, 2), POISON, dtype=torch.int32, device=DEV)
                loss = torch.full((F + 1, 3), float("nan"), device=DEV)
                llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
                stats = torch.full((G + 1, 3), POISON, dtype=torch.int32, device=DEV)
                _lib.check(_entry(p, ops, f, counts, loss, None if off is None else llr.data_ptr() + off, stats.data_ptr() if with_stats else None,
                                  n, hp, ep))
                _same_bits([counts[:F], loss[:F]], want[:2])
                assert (counts[F:] == POISON).all() and loss[F:].isnan().all()
                if with_stats:
                    _same_bits([stats[:G]], [want[3]])
                    assert (stats[G:] == POISON).all()
                else:
                    assert (stats == POISON).all()
                if off is None:
                    assert llr.isnan().all()
                else:
                    at = off // 4
                    _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                    assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
            got = _run(name, m, R, want_llr=False)
            _same_bits([got[0], got[1], got[3]], [want[0], want[1], want[3]])
    # the odd grid whose last element (14, at (2, 4)) is data and alone in its pair: written for both streams, finite and not a pilot's zero
    n, _, ops = _operands(MRC_ODD, 2)
    counts, stats = (torch.full(shape, POISON, dtype=torch.int32, device=DEV) for shape in ((2, 2), (1, 3)))
    loss, llr = torch.full((2, 3), float("nan"), device=DEV), torch.full((2, 3, 5, m), float("nan"), device=DEV)
    _lib.check(_entry(_plan(MRC_ODD, m, 2), ops, f, counts, loss, llr.data_ptr(), stats.data_ptr(), n))
    _same_bits([counts, loss, llr, stats], _run(MRC_ODD, m, 2))
    assert llr.isfinite().all() and (llr[:, 2, 4] != 0).all() and (llr[:, 1, 2] == 0).all()


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_sic_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_sic_f32")
    for m in BITS_PER_SYMBOL:
        for name, R in (("default_120x14", 2), ("odd_30x7", 3), ("odd_30x7", 8), (MRC_ODD, 2)):
            _same_bits(_run(name, m, R, lib=lib), _run(name, m, R))


def test_what_the_plan_refuses():
    n, _, (h, e, k, s, *w) = _operands("odd_30x7", 4)
    p, f, names = _plan("odd_30x7", 4, 4), _dev(FACTORS), ("rho", "scale", "reg")
    swapped = lambda i, t: (h, e, k, s, *w[:i], t, *w[i + 1:], f)  # noqa: E731
    for args, word in (((h[:6], e[:6], k[:6], s[:6], w[0][:6], *w[1:], f), "6 frames is not a multiple of branches \\* streams = 4 \\* 2"),
                       *((swapped(i, w[i][:8 if i == 0 else 3]), f"{names[i]} must hold") for i in range(3)),
                       (swapped(2, w[2].double()), "reg must be torch.float32"),
                       (swapped(2, torch.from_numpy(np.zeros(4, np.float32))), "pinned host memory"),
                       ((h, e, k, s, *w, torch.ones(9, device=DEV)), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            p(*args)
    for bad in (0, 1, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            LinkSicPlan(p.cfg, DEV, bad)
    for bad in (1, 3, 2.0, True):
        with pytest.raises(ValueError, match="streams"):
            LinkSicPlan(p.cfg, DEV, 2, bad)
    with pytest.raises(ValueError, match="LinkSicPlan runs on a HIP device"):
        LinkSicPlan(p.cfg, "cpu", 2)


def test_every_refusal_of_the_entry_point_launches_nothing():
    name, m, R = "default_120x14", 4, 2
    n, _, (h, e, k, s, *w) = _operands(name, R)
    lib, F, f = _lib.load(), n // R, _dev(FACTORS)
    fn, words = lib.aft_link_sic_f32, ("rho", "scale", "reg")
    cfg = LinkConfig(sm_inputs(name)[0], m)
    counts, stats = (torch.full(shape, POISON, dtype=torch.int32, device=DEV) for shape in ((F, 2), (F // 2, 3)))
    loss = torch.full((F, 3), float("nan"), device=DEV)
    llr = torch.full((F, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), **{x: t.data_ptr() for x, t in zip(words, w)},
                factors=f.data_ptr(), n_factors=3, branches=R, streams=2, counts=counts.data_ptr(), loss=loss.data_ptr(),
                llr=llr.data_ptr(), stats=stats.data_ptr(), batch=n)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return fn(ctypes.byref(p), *(a[x] for x in good), None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert fn(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for x in ("ideal", "est", "keys", "sigma", *words, "factors", "counts", "loss"):
        refused(E, "NULL pointer", **{x: None})
    for x in ("ideal", "est", "keys"):
        refused(E, "8-byte", **{x: good[x] + 4})
    for x in ("sigma", *words, "factors", "counts", "loss", "llr", "stats"):
        refused(E, "4-byte", **{x: good[x] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for nf in (0, 9, -1):
        refused(E, f"n_factors = {nf} is outside 1..8", n_factors=nf)
    for bad in (1, 3, 0, -2):
        refused(SH, f"streams = {bad}", streams=bad)
    for bad in (1, 0, 9, -2):
        refused(SH, f"branches = {bad} is outside 2..8", branches=bad)
    refused(E, "batch = 16 is not a multiple of branches * streams = 3 * 2", branches=3)
    refused(E, "batch = 14 is not a multiple of branches * streams = 2 * 2", batch=14)
    for field, value, word in (("num_scs", 0, "num_scs = 0"), ("pilot_scs", 65, "pilot_scs = 65 is outside 1..64"),
                               ("num_symbols", 1, "larger than the ofdm grid"), ("bits_per_symbol", 3, "bits_per_symbol = 3")):
        p = cfg.to_struct()
        setattr(p, field, value)
        refused(SH, word, p=p)
    torch.cuda.synchronize()
    assert (counts == POISON).all() and loss.isnan().all() and llr.isnan().all() and (stats == POISON).all()     # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    _same_bits([counts, loss, llr, stats], _run(name, m, R))                     # ... and the good call writes it all
    # a grid whose every element is a pilot is legal: counts 0, loss 0, LLR 0, stats 0
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), m).to_struct()
    assert call(one, batch=4) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert counts[:2].tolist() == [[0, 0]] * 2 and loss[:2].tolist() == [[0.0] * 3] * 2 and llr.reshape(-1)[:2 * m].tolist() == [0.0] * (2 * m)
    assert stats[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("kind", ("viterbi", "ldpc"))
def test_coded_accumulators_with_sic_run_without_a_synchronisation(kind):
    """``link2_gpu.coded_accumulators`` for ``detector="sic"``: three batches, the last two under the no-synchronisation guard, against the
    host decoders on the LLRs ``LinkSicPlan`` returns for the same operands; ``sic_propagation`` is the sum of those launches' stats."""
    R, N, seed = 2, 2, 2
    sim = ChannelSimConfig()
    link = LinkConfig(sim, 4)
    code = CodeConfig(link, 256, "3/4") if kind == "viterbi" else LdpcConfig(link, "1/2")
    make = BlockErrorAccumulator if kind == "viterbi" else LdpcBlockErrorAccumulator
    decode = link_decode_host if kind == "viterbi" else link_ldpc_host
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=seed)
    with_est, perfect, on_device = (make(code, DEV, seed=seed, branches=R, streams=N, detector="sic") for _ in range(3))
    assert type(with_est._plan) is LinkSicPlan
    it = iter(loader)
    first = next(it)
    seen = []

    def step(batch):
        pil, ideal, meta = batch
        est = model(pil, meta)
        with_est.update(est, ideal, meta)
        perfect.update(None, ideal, meta)
        on_device.update(est, ideal, frame_ids=meta[0].to(DEV, non_blocking=True), snr_db=meta[1])
        seen.append((ideal, est, meta))

    step(first)                                   # the first batch builds the plans and the pinned blocks: outside the guard
    torch.cuda.synchronize()
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                          # the mode is honoured: what follows is not vacuous
        for batch in it:
            step(batch)
    rows = 48 // R                                # G N
    assert len(seen) == 3 and with_est.frames == perfect.frames == rows and with_est.errors.is_cuda
    p, one = LinkSicPlan(link, DEV, R), torch.ones(1, device=DEV)
    want, stats = np.zeros((2, len(with_est.errors)), np.int64), np.zeros((2, 3), np.int64)
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        sent_keys = np.ascontiguousarray(keys.reshape(-1, R, N)[:, 0, :]).reshape(-1)
        w = tuple(_dev(a) for a in sm_weights(snr, 0.0, R, N, "mmse"))
        for i, e in enumerate((est, ideal)):
            _, _, llr, st = p(ideal, e, _dev(keys), _dev(noise_sigma(snr)), *w, one, want_llr=True)
            want[i] += decode(code, sent_keys, llr.cpu().numpy())[0].sum(axis=0)
            stats[i] += st.cpu().numpy().sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()     # keys hashed on the device are the host's
    assert with_est.result() == want[0][1] / (rows * code.blocks) and perfect.result() <= with_est.result()
    elements = rows // N * link.data_elements
    for acc, st in ((with_est, stats[0]), (perfect, stats[1]), (on_device, stats[0])):
        assert acc.sic_propagation() == (st[0] / elements, st[1] / elements, st[2] / st[1] if st[1] else 0.0)
    print(f"{kind}, 2 x 2 sic: BLER with the LMMSE estimate {with_est.result():.3f}, with the channel {perfect.result():.3f}; "
          f"propagation (swapped, first SER, propagated) {with_est.sic_propagation()} / {perfect.sic_propagation()}")


def test_sic_propagation_of_a_device_sweep_is_the_sum_of_the_launches():
    """``LinkAccumulator`` on the inputs of this file, one update per grid's frames: the three shares are the plan's stats summed."""
    name, m, R = "odd_30x7", 6, 4
    sim, keys, sigma, snr, ideal, est = sm_inputs(name)
    cfg = LinkConfig(sim, m)
    acc = LinkAccumulator(cfg, DEV, seed=3, branches=R, streams=2, detector="sic")
    total = np.zeros(3, np.int64)
    for part in (slice(0, 16), slice(16, 32)):
        acc.update(_dev(est["lmmse"][part]), _dev(ideal[part]), frame_ids=np.arange(32)[part], snr_db=snr[part])
        w = tuple(_dev(a) for a in sm_weights(snr[part], 0.0, R, 2, "mmse"))
        total += _plan(name, m, R)(_dev(ideal[part]), _dev(est["lmmse"][part]), _dev(keys[part]), _dev(sigma[part]), *w, _dev(FACTORS))[3] \
            .cpu().numpy().sum(axis=0)
    elements = 32 // (2 * R) * cfg.data_elements
    assert total[1] > 0 and acc.sic_propagation() == (total[0] / elements, total[1] / elements, total[2] / total[1])
    with pytest.raises(ValueError, match="sic_propagation needs"):
        LinkAccumulator(cfg, DEV, seed=3, branches=R, streams=2).sic_propagation()
